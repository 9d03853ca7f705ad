"""Step API of ``pretrain_GeoSSL.py --GeoSSL_option=DDM`` (examples/pretrain_GeoSSL.py:68-74,179-212,
234-260) on the HIP path.

``perturb`` and ``do_DDM`` keep the reference signatures.  The reference reads two module globals
(``NCSN_model_01/02``, :207-208); here they are module attributes with the same names, or can be
passed with ``NCSN_models=``.  ``DDMTrainer`` is the training-loop body (:234-260) with all
parameters in one flat buffer: one fused Adam launch and one RCCL all-reduce per step.

Forward + backward of a step are captured into HIP graphs keyed on a FINGERPRINT of the batch's index structure
(``batch.structure_fingerprint``) and replayed (``replay.StepGraphs``) - by ``DDMTrainer`` and, for a caller that keeps
the reference's own loop (``loss, acc = do_DDM(...); optimizer.zero_grad(); loss.backward(); optimizer.step()``,
:249-260), by ``do_DDM`` itself (``autograd_step._AutogradStep``): the loss it returns is the output of an autograd node
whose backward hands the replayed gradients to autograd.  The batch types, the graph engine and the trainer base are
re-exported from ``batch.py``, ``replay.py``, ``autograd_step.py`` and ``step.py``.

The other options of the script live here too: ``do_InfoNCE`` / ``do_EBM_NCE`` with ``ContrastiveTrainer`` (:103-176) and
``do_RR`` with ``RRTrainer`` (:77-100; its ``AutoEncoder`` heads are this project's own definition,
``Geom3D/models/autoencoder.py``, on the fused kernels of csrc/rr_head.hip).
"""
import numpy as np
import torch
from .switches import env as _env

from . import _lib, ops
from ._lib import call, ptr, stream
from .autograd_step import _AutogradStep, _ReplayedLoss, _StepLoss, _Ticket  # noqa: F401
from .batch import Batch, TripleBatch, _tensor_uid, canonical_option, structure_fingerprint  # noqa: F401
from .layout import MolLayout
from .replay import StepGraphs, _MT_PENDING, _NOISE_KEYS, _restore_backward_threads  # noqa: F401
from .step import (Args, Objective, StepTrainer, _OWN_CAPTURE, draw_target, engine_for, latent, own_capture_open,  # noqa: F401
                   run_graphed, stock_bce, with_counts)

NCSN_model_01 = None
NCSN_model_02 = None


def perturb(x, positions, mu, sigma, noise=None, device_noise=False, generator=None):
    """pretrain_GeoSSL.py:68-74.  Default: the N(mu, sigma) draw is made on the CPU and copied to
    the device exactly like the reference (:72), so the same seed gives the same noise.
    ``device_noise=True`` draws on the GPU instead (no host RNG / PCIe copy); ``noise=`` injects it."""
    x_perturb = x
    device = positions.device
    if noise is None:
        if device_noise:
            noise = torch.empty_like(positions).normal_(mu, sigma, generator=generator)
        else:
            noise = torch.normal(mu, sigma, size=positions.size()).to(device)
    positions_perturb = ops.add_scaled(positions, noise, 1.0)
    return x_perturb, positions_perturb


class _SplitViews(torch.autograd.Function):
    """h of the fused (clean ‖ perturbed) batch -> the two per-view halves.  Plain slicing would make autograd pad each
    half's gradient to the full shape and add the two (two fills, two copies and an add over 2N x F); the backward
    here is one concatenation - or nothing at all when the two gradients already lie behind one another in one buffer,
    which is where the heads put them when the halves carry a `GradSlot` (`split_views`)."""

    STATS = {"adjacent": 0, "cat": 0}  # how the backward joined the halves (tests)

    @staticmethod
    def forward(ctx, h, n):
        ctx.n = n
        return h[:n], h[n:]

    @staticmethod
    def backward(ctx, g1, g2):
        if (g1.is_contiguous() and g2.is_contiguous() and g1.dtype == g2.dtype and g1.dim() == 2
                and g1.untyped_storage().data_ptr() == g2.untyped_storage().data_ptr()
                and g2.storage_offset() == g1.storage_offset() + g1.numel()):
            _SplitViews.STATS["adjacent"] += 1
            return g1.new_empty(0).set_(g1.untyped_storage(), g1.storage_offset(),
                                        (g1.size(0) + g2.size(0), g1.size(1)), (g1.size(1), 1)), None
        _SplitViews.STATS["cat"] += 1
        return torch.cat([g1, g2]), None


class GradSlot:
    """Where a consumer of one half of a split tensor may put that half's gradient: rows [lo, hi) of a buffer the two
    halves share (allocated by whoever asks first).  A head that finds the slot on its input (`_geossl_grad_slot`,
    NCSN._NcsnLoss) writes its gradient there and returns that view; anything else ignores it and `_SplitViews.backward`
    concatenates as before."""

    def __init__(self, pair, lo, hi, total):
        self.pair, self.lo, self.hi, self.total = pair, lo, hi, total

    def rows(self, n, width, dtype, device):
        if n != self.hi - self.lo:
            return None
        buf, given = self.pair.get("buf"), self.pair.setdefault("given", set())
        if (buf is None or self.lo in given  # a second backward through the same graph: never into a buffer handed out
                or buf.shape != (self.total, width) or buf.dtype != dtype or buf.device != device):
            buf = torch.empty(self.total, width, dtype=dtype, device=device)
            self.pair["buf"] = buf
            given.clear()
        given.add(self.lo)
        return buf[self.lo:self.hi]


def split_views(h, n):
    a, b = _SplitViews.apply(h, n)
    pair = {}
    a._geossl_grad_slot = GradSlot(pair, 0, n, h.size(0))
    b._geossl_grad_slot = GradSlot(pair, n, h.size(0), h.size(0))
    return a, b


def _two_view_batch(batch_vec, num_graphs):
    """batch ids of the concatenated (clean ‖ perturbed) 2B-molecule batch + its layout, cached on
    the batch tensor object."""
    cached = getattr(batch_vec, "_geossl_two_view", None)
    if cached is None or cached[2] != batch_vec._version:
        b2 = torch.cat([batch_vec, batch_vec + num_graphs])
        hs = getattr(batch_vec, "_geossl_sizes", None)  # host sizes left by layout.prepare_batch(lazy=True)
        sizes = hs[0] if hs is not None and hs[1] == batch_vec._version and len(hs[0]) == num_graphs else None
        lay2 = MolLayout(b2, 2 * num_graphs, sizes=None if sizes is None else sizes + sizes)
        if sizes is not None and not torch.cuda.is_current_stream_capturing():
            lay2.loop_plan()
        cached = (b2, lay2, batch_vec._version)
        batch_vec._geossl_two_view = cached
    return cached[0], cached[1]


def _two_view_edges(batch_vec, edge_index, num_graphs):
    """(batch ids, radius_edge_index) of the concatenated (clean ‖ perturbed) batch for PaiNN — the perturbed view
    keeps the clean view's graph (PaiNN does not re-derive it) — cached on the edge_index tensor so the
    incidence structures behind it are built once per batch."""
    cached = getattr(edge_index, "_geossl_two_view", None)
    key = (batch_vec._version, edge_index._version)
    if cached is None or cached[2] != key:
        b2 = torch.cat([batch_vec, batch_vec + num_graphs])
        e2 = torch.cat([edge_index, edge_index + batch_vec.numel()], dim=1)
        cached = (b2, e2, key)
        edge_index._geossl_two_view = cached
    return cached[0], cached[1]


def do_DDM(args, batch, model, criterion=None, mu=0.0, sigma=0.3, num_neg=1, NCSN_models=None, noise=None,
           fuse_views=True, device_noise=False, graph=None):
    """pretrain_GeoSSL.py:179-212 -> (loss, 0).

    noise: optional dict with pos_noise [N,3], noise_level_1/2 [B] int64, dist_noise_1/2 [S,1] —
    the five random draws of the step; anything missing is drawn like the reference does.
    fuse_views: run the clean and the perturbed view through the backbone as one 2B-molecule batch
    (molecules never interact, so every row sees the same arithmetic as in two separate calls).
    graph: replay a captured HIP graph of forward + backward (see ``_AutogradStep``) when gradients are wanted and the
    batch's index structure has a fingerprint; default: ``args.step_graph`` if present, else on unless
    ``GEOSSL_NO_STEP_GRAPH`` is set.  The draws, the loss and the gradients are those of the eager path, bit for bit.
    """
    n1, n2 = NCSN_models if NCSN_models is not None else (NCSN_model_01, NCSN_model_02)
    if n1 is None or n2 is None:
        raise RuntimeError("set geossl_amd.pretrain_GeoSSL.NCSN_model_01/02 or pass NCSN_models=(m1, m2)")
    if fuse_views:
        dargs = Args(args.model_3d, bool(getattr(args, "normalize", False)), mu, sigma, device_noise)
        loss = run_graphed(args, graph, model, "_geossl_autograd_step", DDM, dargs, batch, noise, n1, n2)
        if loss is not None:
            return loss, 0
    return _do_ddm_eager(args, batch, model, mu, sigma, (n1, n2), noise, fuse_views, device_noise), 0


def _do_ddm_eager(args, batch, model, mu, sigma, heads, noise, fuse_views, device_noise):
    """The step as eager launches behind autograd's own nodes (one per backbone / head)."""
    noise = noise or {}
    n1, n2 = heads
    positions = batch.positions
    x_01 = batch.x[:, 0]
    positions_01 = positions
    super_edge_index = batch.super_edge_index
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    bucket = getattr(batch, "_bucket", None)
    if bucket is not None:
        # the static batch of a capacity bucket (geossl_amd/bucket.py): tensors have the bucket's capacity, the real counts
        # are device data (bucket.dyn); the fused batch is [view 0 | view 1 | unused] and goes to the heads whole
        if args.model_3d != bucket.kind or not fuse_views or getattr(args, "normalize", False):
            raise _lib.GeosslHipError("capacity buckets serve the fused step of the backbone they were made for")
        pos_noise = noise.get("pos_noise")
        if pos_noise is None:
            pos_noise = torch.empty_like(positions).normal_(mu, sigma)
        pos2, distance_01, distance_02, x2 = ops.ddm_views(positions, pos_noise, super_edge_index[0], super_edge_index[1],
                                                           z=x_01, dyn=bucket.dyn)
        if bucket.kind == "schnet":
            h = latent(model, "schnet", x2, pos2, bucket.b2, layout=bucket.lay2)
        else:
            h = latent(model, "painn", x2, pos2, bucket.b2, bucket.e2, layout=bucket.lay2, edge_layout=bucket.el)
        from .NCSN import ddm_heads_loss
        return ddm_heads_loss(n1, n2, batch, h, distance_02, None, distance_01,
                              noise_level_1=noise.get("noise_level_1"), distance_noise_1=noise.get("dist_noise_1"),
                              noise_level_2=noise.get("noise_level_2"), distance_noise_2=noise.get("dist_noise_2"),
                              out_scale=0.5)
    if fuse_views:
        # perturb (:68-74), the concatenation of the two views and both sets of super-edge lengths (:199-205) in one
        # launch; the draw itself is perturb's (same generator, same place in the order of draws)
        pos_noise = noise.get("pos_noise")
        if pos_noise is None:
            if device_noise:
                pos_noise = torch.empty_like(positions).normal_(mu, sigma)
            else:
                pos_noise = torch.normal(mu, sigma, size=positions.size()).to(positions.device)
        N = positions.size(0)
        pos2, distance_01, distance_02, x2 = ops.ddm_views(positions, pos_noise, super_edge_index[0], super_edge_index[1],
                                                           z=x_01)
        if args.model_3d == "schnet":
            b2, lay2 = _two_view_batch(batch.batch, batch.num_graphs)
            # the readout is dead compute in this step (`_` at pretrain_GeoSSL.py:187): not evaluated
            h = latent(model, "schnet", x2, pos2, b2, layout=lay2)
        else:
            b2, e2 = _two_view_edges(batch.batch, batch.radius_edge_index, batch.num_graphs)
            h = latent(model, "painn", x2, pos2, b2, e2)
        molecule_3D_repr_01, molecule_3D_repr_02 = split_views(h, N)
    else:
        x_02, positions_02 = perturb(x_01, positions, mu, sigma, noise=noise.get("pos_noise"), device_noise=device_noise)
        if args.model_3d == "schnet":
            _, molecule_3D_repr_01 = model(x_01, positions_01, batch.batch, return_latent=True)
            _, molecule_3D_repr_02 = model(x_02, positions_02, batch.batch, return_latent=True)
        else:
            _, molecule_3D_repr_01 = model(x_01, positions_01, batch.radius_edge_index, batch.batch, return_latent=True)
            _, molecule_3D_repr_02 = model(x_02, positions_02, batch.radius_edge_index, batch.batch, return_latent=True)
        distance_01 = ops.pair_distance(positions_01, super_edge_index[0], super_edge_index[1])  # :199-201
        distance_02 = ops.pair_distance(positions_02, super_edge_index[0], super_edge_index[1])  # :203-205

    if getattr(args, "normalize", False):  # :193-195
        molecule_3D_repr_01 = ops.row_normalize(molecule_3D_repr_01)
        molecule_3D_repr_02 = ops.row_normalize(molecule_3D_repr_02)

    # cross-view pairing (:207-208); each head returns 0.5 * its loss so the sum is (l1 + l2) / 2 (:210)
    # (both heads in the same launches where they allow it: NCSN.ddm_heads_loss)
    from .NCSN import ddm_heads_loss
    return ddm_heads_loss(n1, n2, batch, molecule_3D_repr_01, distance_02, molecule_3D_repr_02, distance_01,
                          noise_level_1=noise.get("noise_level_1"), distance_noise_1=noise.get("dist_noise_1"),
                          noise_level_2=noise.get("noise_level_2"), distance_noise_2=noise.get("dist_noise_2"),
                          out_scale=0.5)


_PINNED = {"i": 0, "slots": [[None, None], [None, None]]}  # ring of two pinned staging buffers (grow-only) + copy events


def _host_normal_into(dst, mu, sigma):
    """torch.normal(mu, sigma, size) on the HOST generator (the reference's draw, pretrain_GeoSSL.py:72: same stream, same
    values) into the device tensor `dst` without stalling the host: the draw is made straight into pinned memory and
    copied asynchronously (a pageable source makes the copy wait for everything queued on the stream before it - in the
    reference loop that is the whole previous backward)."""
    key, n = tuple(dst.shape), dst.numel()
    ring = _PINNED
    slot = ring["slots"][ring["i"]]
    ring["i"] ^= 1
    if slot[1] is not None:
        slot[1].synchronize()  # the copy that last read this staging buffer (two steps ago)
    if slot[0] is None or slot[0].numel() < n:
        # one buffer for every size (a shuffled loader's batches all differ: pinning memory per shape cost a step's time)
        slot[0] = torch.empty(max(n + n // 4, 4096), dtype=torch.float32).pin_memory()
    stage = slot[0][:n].view(key)
    torch.normal(mu, sigma, size=key, out=stage)   # (the values of a fresh tensor of this size: the generator fills in order)
    dst.copy_(stage, non_blocking=True)
    slot[1] = torch.cuda.Event()
    slot[1].record()


def draw_step_noise(batch, n1, n2, mu, sigma, device_noise, given=None, into=None):
    """The five random draws of a step in the order the eager path makes them: perturb (pretrain_GeoSSL.py:72: a
    host draw copied to the device, or a device draw with device_noise), then per head the noise level (NCSN.py:190)
    and the distance noise (:194).  Entries of `given` are used instead of drawing; with `into` the results are written
    into those tensors (the static inputs of a graph) instead of new ones."""
    given = given or {}
    if getattr(batch, "_dataset", None) is not None:   # (a dataset handle knows its counts without collated tensors)
        dev, S, B = batch.device, batch.n_super, batch.num_graphs
    else:
        dev = batch.positions.device
        S, B = batch.super_edge_index.size(1), batch.num_graphs
    out = {}

    def put(key, make, fill):
        if given.get(key) is not None:
            if into is not None:
                into[key].copy_(given[key].view_as(into[key]))
            out[key] = into[key] if into is not None else given[key]
        elif into is not None:
            fill(into[key])
            out[key] = into[key]
        else:
            out[key] = make()

    if device_noise:
        put("pos_noise", lambda: torch.empty_like(batch.positions).normal_(mu, sigma), lambda t_: t_.normal_(mu, sigma))
    else:  # the reference's own draw (:72): CPU generator, then the copy
        put("pos_noise", lambda: torch.normal(mu, sigma, size=batch.positions.size()).to(dev),
            lambda t_: _host_normal_into(t_, mu, sigma))
    for k, head in (("1", n1), ("2", n2)):
        K = head.sigmas.size(0)
        put("noise_level_" + k, lambda: torch.randint(0, K, (B,), device=dev), lambda t_: t_.random_(0, K))
        put("dist_noise_" + k, lambda: torch.randn(S, 1, device=dev), lambda t_: t_.normal_())
    return out


def _next_noise_key(dev):
    """A 64-bit Philox key from the state of torch's CUDA generator of this device, taken on the HOST (no launch): the
    generator's seed mixed with its offset, which is then advanced like a draw of four values would - so
    torch.cuda.manual_seed governs the stream and other torch draws in between move it, exactly as when the key was
    drawn on the device."""
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    off = int(gen.get_offset())
    gen.set_offset(off + 4)
    m64 = (1 << 64) - 1
    x = (int(gen.initial_seed()) + 0x9E3779B97F4A7C15 * (off // 4 + 1)) & m64     # splitmix64 of (seed, draw number)
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m64
    return x ^ (x >> 31)


def draw_step_noise_fused(batch, n1, n2, mu, sigma, into=None):
    """The five draws of a step for a caller that owns its random stream (DDMTrainer with device noise): ONE 64-bit key
    derived on the host from torch's CUDA generator (so torch.cuda.manual_seed governs the stream), then one launch that
    fills all five tensors (geossl_ddm_noise_seeded: Philox under that key) - one launch where the torch calls are five.  New tensors, or
    in place into `into` (the static inputs of a graph)."""
    dev = batch.positions.device
    N, S, B = batch.positions.size(0), batch.super_edge_index.size(1), batch.num_graphs
    if into is None:
        into = {"pos_noise": torch.empty(N, 3, dtype=torch.float32, device=dev),
                "noise_level_1": torch.empty(B, dtype=torch.long, device=dev),
                "dist_noise_1": torch.empty(S, 1, dtype=torch.float32, device=dev),
                "noise_level_2": torch.empty(B, dtype=torch.long, device=dev),
                "dist_noise_2": torch.empty(S, 1, dtype=torch.float32, device=dev)}
    for k in _NOISE_KEYS:
        assert into[k].is_contiguous()
    call("geossl_ddm_noise_seeded", _next_noise_key(dev), float(mu), float(sigma), 3 * N, S, B, n1.sigmas.size(0), n2.sigmas.size(0),
         ptr(into["pos_noise"]), ptr(into["noise_level_1"]), ptr(into["dist_noise_1"]), ptr(into["noise_level_2"]),
         ptr(into["dist_noise_2"]), stream())
    return into


def _ddm_forward(owner, args, batch, noise):
    return _do_ddm_eager(args, batch, owner.model, args.mu, args.sigma, (owner.n1, owner.n2), noise, True,
                         args.device_noise)


def _ddm_head_params(head):
    from .NCSN import _head_params
    return _head_params(head)


def _ddm_write(owner, args, g, batch, noise):
    on, into = draw_target(owner, g, batch, noise)
    draw_step_noise(on, owner.n1, owner.n2, args.mu, args.sigma, args.device_noise, noise, into=into)


# the five draws of a step are the static inputs of its graphs: made for a capture, drawn into them before a replay
# (whatever the caller gave is copied instead of drawn)
DDM = Objective(
    "DDM", _ddm_forward, views=2, normalize=True, head_params=_ddm_head_params,
    graph_key=lambda args: (args.model_3d, bool(getattr(args, "normalize", False))),
    noise_keys=lambda args: _NOISE_KEYS,
    capture_inputs=lambda owner, args, batch, noise:
        draw_step_noise(batch, owner.n1, owner.n2, args.mu, args.sigma, args.device_noise, noise),
    write_inputs=_ddm_write)


class DDMTrainer(StepTrainer):
    """The body of ``train()`` (pretrain_GeoSSL.py:234-260) for the DDM option: forward of both
    views + both heads, backward, gradient all-reduce, Adam — flat parameter buffer, no host sync
    inside ``step`` (the reference's per-step ``loss.item()`` at :255 is logging, call
    ``float(loss)`` outside the timed region if wanted).

    ``use_graph=True``: forward + backward are captured once per index structure into a HIP graph and replayed;
    positions, atom types and the five noise tensors are copied into the graph's static buffers before each replay
    (with ``noise=None`` and ``device_noise=True`` the trainer makes the five draws itself, straight into those
    buffers).  Which graph a batch gets is decided by ``structure_fingerprint`` - the molecule sizes for batches whose
    index tensors are a function of them, the tensor objects otherwise - never by the caller: a shuffled loader with
    ragged molecules captures one graph per distinct size sequence (up to ``max_graphs``, least recently used dropped,
    all in one shared memory pool).  The all-reduce and the Adam launch stay outside the graph."""

    def __init__(self, model, ncsn_01, ncsn_02, lr=5e-4, weight_decay=0.0, mu=0.0, sigma=0.3, model_3d="schnet",
                 device_noise=True, use_graph=False, overlap_heads=True, max_graphs=256, graph_mode="auto"):
        # two-pass NCSN backward only (GEOSSL_NCSN_SPLIT_BWD): its weight-gradient kernels on a side stream, concurrent
        # with the backbone's backward; the default one-pass backward has nothing to overlap
        self.overlap_heads = overlap_heads
        self._zero_outside = True
        self._side = None
        super().__init__([model, ncsn_01, ncsn_02], DDM, Args(model_3d, False, mu, sigma, device_noise), lr, weight_decay,
                         use_graph, max_graphs, graph_mode)

    @property
    def _graphs(self):
        return self.step_graphs.graphs

    # DDMTrainer's own: the gradient buffer is cleared by the step itself unless `_zero_outside` leaves it to its own
    # capture's refresh, and the step's device draws are the trainer's (`_draw_noise`), eager or replayed alike
    def _fwd_bwd(self, batch, noise):
        if not (self._zero_outside and own_capture_open()):
            self.flat.zero_grad()  # (a replayed step: cleared with the refresh of the graph's inputs, StepGraphs.refresh)
        if noise is None and self.args.device_noise:
            noise = self._draw_noise(batch)  # the trainer's own stream, eager launches or replayed graph alike
        return self._backward(self._forward(batch, noise))

    # DDMTrainer's own: the heads' weight gradients on the NCSN side stream
    def _backward(self, loss):
        from . import NCSN as _ncsn
        if self._side is None and self.overlap_heads:
            self._side = torch.cuda.Stream()
        _ncsn.set_side_stream(self._side)  # head weight gradients overlap the backbone's backward
        try:
            with _lib.direct_grads():  # every p.grad is a view of self.flat.grad: kernels accumulate into it directly
                loss.backward(self._one)  # (a standing 1.0: backward() would fill a new one, a launch per step)
        finally:
            _ncsn.set_side_stream(None)
            _ncsn.join_side_stream()
        self.flat.rebind_grads()
        return loss.detach()

    _NOISE_KEYS = _NOISE_KEYS

    # DDMTrainer's own: its device draws are ONE seeded launch (`_draw_noise`), where DDM's hooks - the engine's - make
    # torch's five; a caller's noise takes the hooks
    def _capture_inputs(self, batch, noise):
        return self._draw_noise(batch) if noise is None else super()._capture_inputs(batch, noise)

    def _write_inputs(self, g, batch, noise):
        if noise is None:  # straight into the graph's static inputs (g["batch"]: a bucket's draws cover its capacity)
            self._draw_noise(g["batch"], into=g["noise"])
        else:
            super()._write_inputs(g, batch, noise)

    def _draw_noise(self, batch, into=None):
        """The five random draws of a step on the device (perturb: pretrain_GeoSSL.py:72; the heads: NCSN.py:190,194),
        as tensors - new ones, or in place into `into`."""
        a = self.args
        if _env("GEOSSL_TORCH_DRAWS"):  # the five torch calls (the form before geossl_ddm_noise)
            return draw_step_noise(batch, self.n1, self.n2, a.mu, a.sigma, True, None, into)
        return draw_step_noise_fused(batch, self.n1, self.n2, a.mu, a.sigma, into)

    def step(self, batch, noise=None, structure_key=None):
        """One training step.  ``structure_key`` is accepted for compatibility and ignored: graphs are found by the
        batch's own fingerprint.  A ``noise`` that lacks one of the five draws runs eagerly (the rest is drawn there)."""
        if noise is not None and not all(k in noise for k in _NOISE_KEYS):
            return self._finish(self._eager(batch, noise))
        return super().step(batch, noise)


# ---- the contrastive objectives: --GeoSSL_option=InfoNCE / EBM_NCE (pretrain_GeoSSL.py:103-176) -----------------------
# The reference's do_InfoNCE reads the module global CE_criterion (:165, :345) and ignores its `criterion` argument;
# do_EBM_NCE applies `criterion` (the loop passes nn.BCEWithLogitsLoss(), :344).  A caller may replace CE_criterion like
# NCSN_model_01/02; a criterion other than the stock one runs on the eager fallback (_contrastive_with_criterion).
CE_criterion = torch.nn.CrossEntropyLoss()

CONTRASTIVE_OPTIONS = ("InfoNCE", "EBM_NCE")


class ContrastiveArgs:
    """The fields do_InfoNCE / do_EBM_NCE read from the reference's argparse namespace (examples/config.py:171-172: T
    0.1, normalize off) plus num_neg, which the reference passes as an argument."""

    def __init__(self, model_3d="schnet", normalize=False, T=0.1, num_neg=1, mu=0.0, sigma=0.3, device_noise=True):
        self.model_3d, self.normalize, self.T, self.num_neg = model_3d, bool(normalize), float(T), int(num_neg)
        self.mu, self.sigma, self.device_noise = mu, sigma, device_noise   # perturb's draw (step.Args)


def _stock_ce(c):
    """nn.CrossEntropyLoss() as the reference builds it (:345): what the InfoNCE kernels compute."""
    return (type(c) is torch.nn.CrossEntropyLoss and c.weight is None and c.reduction == "mean"
            and float(c.label_smoothing) == 0.0 and c.ignore_index < 0)


def _stock_bce(c):
    """nn.BCEWithLogitsLoss() as the reference builds it (:344), or None: what the EBM-NCE kernels compute."""
    return stock_bce(c, or_none=True)


def draw_views_noise(batch, mu, sigma, device_noise, given=None, into=None):
    """The one random draw of a contrastive step, perturb's (pretrain_GeoSSL.py:72): a host draw copied to the device, or
    a device draw with device_noise; `given["pos_noise"]` instead of drawing; `into`: written into those tensors."""
    given = given or {}
    src = given.get("pos_noise")
    if into is not None:
        t_ = into["pos_noise"]
        if src is not None:
            t_.copy_(src.view_as(t_))
        elif device_noise:
            t_.normal_(mu, sigma)
        else:
            _host_normal_into(t_, mu, sigma)
        return into
    if src is None:
        if device_noise:
            src = torch.empty_like(batch.positions).normal_(mu, sigma)
        else:
            src = torch.normal(mu, sigma, size=batch.positions.size()).to(batch.positions.device)
    return {"pos_noise": src}


def _contrastive_views(args, batch, model, mu, sigma, noise, device_noise):
    """The readouts of both views (:117-118 / :150-156 with perturb, :68-74) -> (X, Y), each [B, F]: the two views as one
    fused 2B-molecule batch through the backbone (molecules never interact: every row sees the arithmetic of two
    separate calls), the readout of all 2B molecules, the row normalisation of --normalize, then the split."""
    if args.model_3d not in ("schnet", "painn"):
        raise Exception("3D model {} not included.".format(args.model_3d))
    noise = noise or {}
    positions = batch.positions
    x_01 = batch.x[:, 0]
    pos_noise = draw_views_noise(batch, mu, sigma, device_noise, noise)["pos_noise"]
    B = batch.num_graphs
    bucket = getattr(batch, "_bucket", None)
    if bucket is not None:
        # the static batch of a capacity bucket: atom rows at the bucket's capacity (real counts in bucket.dyn, view 1 at
        # row dims[N]); the two-view mol_ptr holds the real offsets of all 2B molecules, so the readout over bucket.lay2
        # and everything after it (2B rows) see exact counts
        if args.model_3d != bucket.kind:
            raise _lib.GeosslHipError("capacity buckets serve the fused step of the backbone they were made for")
        pos2, x2 = ops.two_views(positions, pos_noise, x_01, dyn=bucket.dyn)
        if bucket.kind == "schnet":
            h = model(x2, pos2, bucket.b2, layout=bucket.lay2)
        else:
            h = model(x2, pos2, bucket.e2, bucket.b2, layout=bucket.lay2, edge_layout=bucket.el)
        if getattr(args, "normalize", False):
            h = ops.row_normalize(h)
        return split_views(h, B)
    pos2, x2 = ops.two_views(positions, pos_noise, x_01)
    if args.model_3d == "schnet":
        b2, lay2 = _two_view_batch(batch.batch, B)
        h = model(x2, pos2, b2, layout=lay2)
    else:
        b2, e2 = _two_view_edges(batch.batch, batch.radius_edge_index, B)
        h = model(x2, pos2, e2, b2)
    if getattr(args, "normalize", False):   # F.normalize(dim=-1) is per row: the 2B rows at once
        h = ops.row_normalize(h)
    return split_views(h, B)


def _contrastive_eager(objective, args, batch, model, mu, sigma, noise, device_noise):
    """The step as eager launches -> (loss, counts [2] int32 on the device)."""
    X, Y = _contrastive_views(args, batch, model, mu, sigma, noise, device_noise)
    if objective == "InfoNCE":
        return ops.infonce_loss(X, Y, getattr(args, "T", 0.1))
    return ops.ebm_nce_loss(X, Y, getattr(args, "num_neg", 1))


def contrastive_acc(objective, counts, B, num_neg=1):
    """The reference's acc from the two counts: InfoNCE (:170-175) a mean of two Python floats, EBM-NCE (:136-137) an
    fp32 tensor division turned into a Python float."""
    c0, c1 = int(counts[0]), int(counts[1])
    if objective == "InfoNCE":
        return (c0 * 1. / B + c1 * 1. / B) / 2
    return float(np.float32(c0 + c1) / np.float32(B * (1 + num_neg)))


def _contrastive_with_criterion(objective, args, batch, model, criterion, mu, sigma, num_neg, noise, device_noise):
    """A criterion other than the stock one (weights, pos_weight, label smoothing, another reduction, a subclass): the
    caller's criterion applied to our backbone's readouts in ATen, exactly as the reference writes the loss.  Correct, not
    fast: no graph, no loss kernel."""
    X, Y = _contrastive_views(args, batch, model, mu, sigma, noise, device_noise)
    B = X.size(0)
    dev = X.device
    if objective == "InfoNCE":
        T = getattr(args, "T", 0.1)
        labels = torch.arange(B).long().to(dev)

        def cal_loss(A, Bm):
            logits = torch.div(torch.mm(A, Bm.transpose(1, 0)), T)
            pred = logits.argmax(dim=1, keepdim=False)
            return criterion(logits, labels), pred.eq(labels).sum().detach().cpu().item() * 1. / B
        l1, a1 = cal_loss(X, Y)
        l2, a2 = cal_loss(Y, X)
        return (l1 + l2) / 2, (a1 + a2) / 2
    if not 1 <= num_neg <= B:
        raise ValueError("num_neg must lie in [1, B] (B = %d), got %d" % (B, num_neg))
    shift = lambda k: (torch.arange(B) + k) % B   # cycle_index(B, k), examples/util.py:19-22
    X_neg = X.repeat((num_neg, 1))
    Y_neg = torch.cat([Y[shift(k + 1).to(dev)] for k in range(num_neg)], dim=0)
    pred_pos = torch.sum(X * Y, dim=1)
    pred_neg = torch.sum(X_neg * Y_neg, dim=1)
    loss_pos = criterion(pred_pos.double(), torch.ones(B).to(dev).double())
    loss_neg = criterion(pred_neg.double(), torch.zeros(B * num_neg).to(dev).double())
    loss = (loss_pos + num_neg * loss_neg) / (1 + num_neg)
    acc = (torch.sum(pred_pos > 0).float() + torch.sum(pred_neg < 0).float()) / (len(pred_pos) + len(pred_neg))
    return loss, acc.detach().item()


def _contrastive_objective(option):
    """The step.Objective of one contrastive option: no heads (the readout is part of the step), two views, capacity
    buckets whatever `normalize` says (the row normalisation is over the 2B readout rows, an exact count), one static
    draw; a graph binds T and num_neg (by-value arguments of its loss launches); -> (loss, counts)."""
    def key(args):
        return (option, args.model_3d, bool(getattr(args, "normalize", False)), float(getattr(args, "T", 0.1)),
                int(getattr(args, "num_neg", 1)))

    return Objective(
        option, lambda owner, args, batch, noise:
            _contrastive_eager(option, args, batch, owner.model, args.mu, args.sigma, noise, args.device_noise),
        views=2, graph_key=key, noise_keys=lambda args: ("pos_noise",), capture_inputs=_capture_views_noise,
        write_inputs=_write_views_noise, result=with_counts)


# the one draw of a two-view step (the contrastive options, RR), perturb's, is the static input of its graphs
def _capture_views_noise(owner, args, batch, noise):
    return draw_views_noise(batch, args.mu, args.sigma, args.device_noise, noise)


def _write_views_noise(owner, args, g, batch, noise):
    on, into = draw_target(owner, g, batch, noise)
    draw_views_noise(on, args.mu, args.sigma, args.device_noise, noise, into=into)


INFONCE, EBM_NCE = (_contrastive_objective(o) for o in CONTRASTIVE_OPTIONS)


def _do_contrastive(obj, args, batch, model, criterion, mu, sigma, num_neg, noise, device_noise, graph):
    objective = obj.name
    stock = _stock_ce(CE_criterion) if objective == "InfoNCE" else _stock_bce(criterion)
    if not stock:
        crit = CE_criterion if objective == "InfoNCE" else criterion
        return _contrastive_with_criterion(objective, args, batch, model, crit, mu, sigma, num_neg, noise, device_noise)
    cargs = ContrastiveArgs(args.model_3d, getattr(args, "normalize", False), getattr(args, "T", 0.1), num_neg, mu, sigma,
                            device_noise)
    out = run_graphed(args, graph, model, "_geossl_contrastive_step_" + objective, obj, cargs, batch, noise)
    if out is not None:
        loss, counts = out
        return loss, contrastive_acc(objective, counts, batch.num_graphs, num_neg)
    loss, counts = _contrastive_eager(objective, cargs, batch, model, mu, sigma, noise, device_noise)
    return loss, contrastive_acc(objective, counts.tolist(), batch.num_graphs, num_neg)


def do_InfoNCE(args, batch, model, criterion=None, mu=0.0, sigma=0.3, num_neg=1, noise=None, device_noise=False,
               graph=None):
    """pretrain_GeoSSL.py:141-176 -> (loss, acc): loss an fp32 scalar tensor, acc a Python float.  `criterion` and
    `num_neg` are ignored like in the reference (it uses the module global CE_criterion).  noise: optional
    {"pos_noise": [N, 3]}; device_noise / graph as in do_DDM (graph: HIP graphs of forward + backward, capacity buckets included)."""
    return _do_contrastive(INFONCE, args, batch, model, criterion, mu, sigma, num_neg, noise, device_noise, graph)


def do_EBM_NCE(args, batch, model, criterion=None, mu=0.0, sigma=0.3, num_neg=1, noise=None, device_noise=False,
               graph=None):
    """pretrain_GeoSSL.py:103-138 -> (loss, acc): loss a float64 scalar tensor, acc a Python float.  criterion: None or
    the reference's nn.BCEWithLogitsLoss() run on the kernels; any other criterion on the eager fallback."""
    return _do_contrastive(EBM_NCE, args, batch, model, criterion, mu, sigma, int(num_neg), noise, device_noise,
                           graph)


class ContrastiveTrainer(StepTrainer):
    """The body of ``train()`` (pretrain_GeoSSL.py:234-260) for --GeoSSL_option InfoNCE / EBM_NCE: forward of both views,
    readout, contrastive loss, backward, gradient all-reduce, Adam - all parameters in one flat buffer (one fused Adam
    launch, one all-reduce), like DDMTrainer.  ``step(batch) -> (loss, counts)``: both device tensors, no host sync
    (contrastive_acc turns the counts into the reference's acc).  ``use_graph=True``: forward + backward of a batch
    structure are captured into a HIP graph and replayed (StepGraphs: ragged batches and DeviceLoader handles share one
    capacity-bucket graph per batch size, gathered into its static inputs on the device; the position noise drawn into
    them)."""

    def __init__(self, model, option="InfoNCE", lr=5e-4, weight_decay=0.0, mu=0.0, sigma=0.3, T=0.1, num_neg=1,
                 normalize=False, model_3d="schnet", device_noise=True, use_graph=False, max_graphs=256,
                 graph_mode="auto"):
        if option not in CONTRASTIVE_OPTIONS:
            raise ValueError("option is one of %s" % (CONTRASTIVE_OPTIONS,))
        self.option = option
        # (capacity buckets with no heads; `normalize` is over the 2B readout rows and does not keep a batch off them;
        # EBM-NCE's loss is a float64 scalar: so is the standing 1.0 of its backward)
        super().__init__([model], INFONCE if option == "InfoNCE" else EBM_NCE,
                         ContrastiveArgs(model_3d, normalize, T, num_neg, mu, sigma, device_noise), lr, weight_decay,
                         use_graph, max_graphs, graph_mode,
                         one_dtype=torch.float64 if option == "EBM_NCE" else torch.float32)

    with_extra = True   # step(batch, noise=None) -> (loss, counts)


# ---- representation reconstruction: --GeoSSL_option=RR (pretrain_GeoSSL.py:77-100) --------------------------------------
# The reference's do_RR reads the module globals AE_model_01/02 (:95-96, built at :320-321); here they are module
# attributes with the same names, or can be passed with ``AE_models=``.  The AutoEncoder class itself is THIS PROJECT'S
# definition (Geom3D/models/autoencoder.py): the reference tree does not contain one.
AE_model_01 = None
AE_model_02 = None


class RRArgs:
    """The fields do_RR reads from the reference's argparse namespace (model_3d, normalize) and what a graph of the step
    binds beside them: the heads' loss kind and ``detach_target`` (config.py:177-183) and the addresses of their
    BatchNorm buffers (the kernels update them in place)."""

    def __init__(self, model_3d="schnet", normalize=False, heads=None, mu=0.0, sigma=0.3, device_noise=True):
        self.model_3d, self.normalize = model_3d, bool(normalize)
        self.heads_key = None if heads is None else _rr_heads_key(heads)
        self.mu, self.sigma, self.device_noise = mu, sigma, device_noise   # perturb's draw (step.Args)


def _rr_bn(head):
    return head.fc_layers[1]


def _rr_buffers(head):
    bn = _rr_bn(head)
    return [bn.running_mean, bn.running_var, bn.num_batches_tracked]


def _rr_heads_key(heads):
    return tuple((h.loss, bool(h.detach_target), float(_rr_bn(h).eps), float(_rr_bn(h).momentum))
                 + tuple(b.data_ptr() for b in _rr_buffers(h)) for h in heads)


def fused_head_ok(head):
    """This project's AutoEncoder (not a subclass) as the fused kernels compute it: training mode, width 128,
    fc_layers = Linear, stock BatchNorm1d with affine parameters, running statistics and a momentum, ReLU, Linear; one of
    the three losses; contiguous fp32 CUDA parameters that all require a gradient."""
    from .Geom3D.models.autoencoder import AE_LOSSES, AutoEncoder
    nn = torch.nn
    if type(head) is not AutoEncoder or not head.training or head.loss not in AE_LOSSES:
        return False
    fc = getattr(head, "fc_layers", None)
    if type(fc) is not nn.Sequential or [type(m) for m in fc] != [nn.Linear, nn.BatchNorm1d, nn.ReLU, nn.Linear]:
        return False
    bn = fc[1]
    if not (bn.affine and bn.track_running_stats and bn.momentum is not None and bn.training and fc[0].training
            and bn.running_mean is not None and bn.num_batches_tracked is not None and bn.running_mean.is_cuda
            and bn.running_mean.dtype == torch.float32 and bn.num_batches_tracked.dtype == torch.long):
        return False
    F_ = head.emb_dim
    shapes = [(F_, F_), (F_,), (F_,), (F_,), (F_, F_), (F_,)]
    ps = list(head.parameters())
    if [tuple(p.shape) for p in ps] != shapes or fc[0].bias is None or fc[3].bias is None:
        return False
    if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.requires_grad for p in ps):
        return False
    return ops.rr_head_width_ok(F_)


def fused_heads_ok(a, b):
    """Two DISTINCT fused-ok AutoEncoders with the same loss and ``detach_target`` and no parameter or buffer in common:
    what one set of launches serves."""
    if a is None or b is None or a is b or not (fused_head_ok(a) and fused_head_ok(b)):
        return False
    if a.loss != b.loss or bool(a.detach_target) != bool(b.detach_target) or a.emb_dim != b.emb_dim:
        return False
    mine = {t.data_ptr() for t in list(a.parameters()) + _rr_buffers(a)}
    return not (mine & {t.data_ptr() for t in list(b.parameters()) + _rr_buffers(b)})


def rr_heads_aten(a, b, X, Y):
    """:95-97 as the reference writes them, on the heads' own ATen forward."""
    AE_loss_1 = a(X, Y)
    AE_loss_2 = b(Y, X)
    return (AE_loss_1 + AE_loss_2) / 2


def rr_heads_loss(a, b, X, Y):
    """(AE_1(X, Y) + AE_2(Y, X)) / 2 -> fp32 scalar: both heads in the fused launches (csrc/rr_head.hip) where
    ``fused_heads_ok`` holds and X, Y are fp32 CUDA rows of the heads' width with B >= 2; the ATen lines otherwise (eval
    mode, other widths, subclasses, CPU tensors; B = 1 in training mode raises torch's own ValueError there)."""
    if (fused_heads_ok(a, b) and X.is_cuda and Y.is_cuda and X.dtype == Y.dtype == torch.float32 and X.dim() == 2
            and X.shape == Y.shape and X.size(1) == a.emb_dim and X.size(0) >= 2):
        buffers = _rr_buffers(a) + _rr_buffers(b)
        from .replay import warming_up
        if warming_up():   # a pass that is no step of the caller's: the running statistics stay where they are
            buffers = [t.clone() for t in buffers]
        bn = tuple((float(_rr_bn(h).eps), float(_rr_bn(h).momentum)) for h in (a, b))
        return ops.rr_heads(X, Y, a.loss, bool(a.detach_target), bn, buffers, list(a.parameters()) + list(b.parameters()))
    return rr_heads_aten(a, b, X, Y)


def _rr_eager(args, batch, model, mu, sigma, heads, noise, device_noise):
    """The step as eager launches: both views through the backbone as one fused batch, readout, --normalize, the split
    (``_contrastive_views``), then the two heads."""
    X, Y = _contrastive_views(args, batch, model, mu, sigma, noise, device_noise)
    return rr_heads_loss(heads[0], heads[1], X, Y)


def rr_step_aten(args, batch, model, AE_models, mu=0.0, sigma=0.3, noise=None, device_noise=False):
    """The step with the heads in ATen whatever they are (the restatement the kernels are tested against, and the route
    of everything they refuse)."""
    X, Y = _contrastive_views(args, batch, model, mu, sigma, noise, device_noise)
    return rr_heads_aten(AE_models[0], AE_models[1], X, Y)


RR = Objective(
    "RR", lambda owner, args, batch, noise:
        _rr_eager(args, batch, owner.model, args.mu, args.sigma, (owner.n1, owner.n2), noise, args.device_noise),
    views=2,
    graph_key=lambda args: ("RR", args.model_3d, bool(getattr(args, "normalize", False)), getattr(args, "heads_key", None)),
    noise_keys=lambda args: ("pos_noise",), capture_inputs=_capture_views_noise, write_inputs=_write_views_noise)


def do_RR(args, batch, model, mu=0.0, sigma=0.3, AE_models=None, noise=None, device_noise=False, graph=None, **kwargs):
    """pretrain_GeoSSL.py:77-100 -> (AE_loss fp32 scalar tensor, 0).  The heads are ``AE_models=(a, b)`` or the module
    globals ``AE_model_01/02``; further keywords (the loop passes ``criterion=``, :246-248) are ignored like in the
    reference.  noise: optional {"pos_noise": [N, 3]}; device_noise / graph as in do_DDM: with two fused-ok heads forward +
    backward replay from HIP graphs (capacity buckets included; the heads' BatchNorm buffers move once per step, eager or
    replayed), and the loss supports the reference's own ``loss.backward()`` with a stock ``torch.optim.Adam``."""
    a, b = AE_models if AE_models is not None else (AE_model_01, AE_model_02)
    if a is None or b is None:
        raise RuntimeError("set geossl_amd.pretrain_GeoSSL.AE_model_01/02 or pass AE_models=(a, b)")
    if fused_heads_ok(a, b) and batch.num_graphs >= 2:
        rargs = RRArgs(args.model_3d, getattr(args, "normalize", False), (a, b), mu, sigma, device_noise)
        loss = run_graphed(args, graph, model, "_geossl_rr_step", RR, rargs, batch, noise, a, b)
        if loss is not None:
            return loss, 0
    return _rr_eager(args, batch, model, mu, sigma, (a, b), noise, device_noise), 0


class RRTrainer(StepTrainer):
    """The body of ``train()`` (pretrain_GeoSSL.py:234-260) for --GeoSSL_option RR: both views through the backbone as
    one fused batch, readout, the two AutoEncoder heads in fused launches, backward, gradient all-reduce, Adam -
    ``[model, ae1, ae2]`` in one flat buffer, no host sync inside ``step(batch, noise=None) -> loss``.

    ``use_graph=True``: forward + backward are captured into HIP graphs and replayed (StepGraphs: ragged batches and
    DeviceLoader handles share one two-view capacity-bucket graph per batch size; the position noise is drawn into the
    graph's static input; the heads' BatchNorm buffers are updated in place by the replayed kernels).

    ``ae_lr=None``: the heads run at the backbone's ``lr`` (one Adam launch).  The reference's loop gives the two AE
    groups ``lr = args.gnn_2d_lr_scale`` (:335-337: the scale itself, 1.0 by default); pass it as ``ae_lr`` for that
    schedule - a second ``geossl_adam_step`` launch over the heads' range of the flat buffer.

    Under data parallelism the gradients are all-reduced like the other trainers'; the BatchNorm batch statistics stay
    PER RANK, as with DistributedDataParallel without SyncBatchNorm (each rank's running statistics follow its own
    batches)."""

    def __init__(self, model, ae_01, ae_02, lr=5e-4, weight_decay=0.0, mu=0.0, sigma=0.3, normalize=False,
                 model_3d="schnet", device_noise=True, use_graph=False, max_graphs=256, graph_mode="auto", ae_lr=None):
        if not fused_heads_ok(ae_01, ae_02):
            raise ValueError("RRTrainer needs two distinct AutoEncoders of width 128 in training mode on the GPU with the "
                             "same loss and detach_target; use do_RR for anything else")
        super().__init__([model, ae_01, ae_02], RR, RRArgs(model_3d, normalize, None, mu, sigma, device_noise), lr,
                         weight_decay, use_graph, max_graphs, graph_mode)
        self.ae_lr = ae_lr
        self._n_backbone = sum(p.numel() for p in model.parameters() if p.requires_grad)

    # RRTrainer's own: two learning rates, the backbone's and the heads'
    def set_lr(self, lr, ae_lr=None):
        """The learning rate of the next steps (a scheduler's value); ae_lr: the heads' (None: unchanged)."""
        self.opt.lr = lr
        if ae_lr is not None:
            self.ae_lr = ae_lr

    def _finish(self, out):
        if self.ae_lr is None or float(self.ae_lr) == float(self.opt.lr):
            return super()._finish(out)
        _lib.poll_status(self.model)
        scale = self.reduce()
        opt, fp, nb = self.opt, self.flat, self._n_backbone
        opt.step_count += 1
        for lo, hi, lr in ((0, nb, opt.lr), (nb, fp.numel, self.ae_lr)):   # the backbone's range, then the heads'
            call("geossl_adam_step", ptr(fp.flat[lo:hi]), ptr(fp.grad[lo:hi]), ptr(opt.exp_avg[lo:hi]),
                 ptr(opt.exp_avg_sq[lo:hi]), hi - lo, float(lr), float(opt.betas[0]), float(opt.betas[1]), float(opt.eps),
                 float(opt.weight_decay), opt.step_count, float(scale), stream())
        return out
