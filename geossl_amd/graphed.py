"""Inference through replayed HIP graphs: ``SchNet.forward(z, pos, batch)`` under ``no_grad`` (the evaluation loops of the
reference: examples/finetune_qm9.py:278-384 ``eval()``; BASELINE config 2, forward only) as ONE graph launch per call.

Launched eagerly a forward pass is ~40 C-ABI calls, and at 1024 molecules per batch the host needs longer to issue them
than the GPU to run them (0.31 of 0.53 ms per pass were launch gaps).  A captured pass also takes the layer loop (the
chains and aggregations of the backbone as one launch, ``ops.layer_loop``), which only pays under capture.

A graph binds the batch's index structure: batches whose index tensors are a function of the molecule sizes (host
sizes known, ``batch.structure_fingerprint``) share a graph per size sequence, captured at the first sighting
for equal-sized molecules and at the second for ragged ones (a loader that never repeats a size sequence never pays for
a capture); everything else runs eagerly.  The result is the graph's static output: valid until the next call (clone it
to keep it).  ``GraphedForward`` and ``ForceTrainer`` are ``replay.StructureGraphs``: its docstring says how they differ.
"""
import torch

from . import _lib, bucket as bk, ops
from .batch import structure_fingerprint
from .layout import get_layout
from .optim import FlatParams, FusedAdam
from .replay import StructureGraphs, capture, copy_static, owned_batch_vector, sizes_key, tensors_key, warm_up


class GraphedForward(StructureGraphs):
    def __init__(self, model, return_latent=False, max_graphs=64):
        super().__init__(max_graphs)
        self.model, self.return_latent = model, return_latent

    def _eager(self, x, positions, batch_vec):
        with torch.no_grad():
            z = x if x.dim() == 1 else x[:, 0]   # (1-D x: a batch of DatasetMD17 / finetune_md17.py's format)
            return self.model(z, positions, batch_vec, return_latent=self.return_latent)

    def __call__(self, batch):
        fp = structure_fingerprint(batch, "schnet") if self.enabled and batch.positions.is_cuda else None
        hit = (fp is not None and fp[0] == "sizes"
               and self.lookup(fp, lambda: bk.is_uniform(batch), lambda: self._capture(batch)))
        if not hit or batch.x.shape != hit[0]["x"].shape:   # (1-D against 2-D x: byte copies would overrun)
            return self._eager(batch.x, batch.positions, batch.batch)
        g, made = hit
        if not made:   # (a new graph's static inputs are clones of this batch)
            copy_static([(g["x"], batch.x), (g["pos"], batch.positions)])
        g["graph"].replay()
        _lib.poll_status(self.model)
        return g["out"]

    def _capture(self, batch):
        x, pos, bvec = batch.x.clone(), batch.positions.clone(), owned_batch_vector(batch.batch)

        def passes():   # (cached layouts, kernel attributes, the loop's block plan)
            self._eager(x, pos, bvec)
            get_layout(bvec).loop_plan()
        warm_up(passes)
        with capture(self, "the forward pass", "enabled") as cap:
            graph, out = cap.record(lambda: self._eager(x, pos, bvec))
        if not cap.ok:
            return None
        return dict(graph=graph, x=x, pos=pos, out=out, batch_vec=bvec, layout=get_layout(bvec))


class ForceTrainer(StructureGraphs):
    """The training step of examples/finetune_md17.py:30-54 - energy head on the backbone's representation, predicted
    force = -dE/dpos taken with ``create_graph=True`` (:46), loss on energy and force (:46-51), ``loss.backward()``
    through the force (:53), ``optimizer.step()`` (:54) - on the library's second-order tape, with the whole of forward,
    position gradient, loss and second-order backward replayed as ONE captured HIP graph per batch structure.

    Launched eagerly such a step is ~1000 C-ABI calls of 10-15 us of host time each: host-bound by a factor of three or
    more.  The tape's launch sequence is a pure function of the batch's index structure, so it is
    captured once and replayed with new atom types, positions and targets copied into the graph's static inputs.

    Which batches share a graph: SchNet derives its graph from the positions inside the kernels (pair-slot form: no edge
    count reaches the host), so every batch with the same molecule sizes in the same order replays one graph - MD17
    (one molecule, a fixed batch size) never captures twice.  PaiNN takes the precomputed ``radius_edge_index`` as an
    input whose length the graph binds: a graph is replayed for batches whose edge tensor is the very same object
    (device-resident pre-collated batches that come back); anything else runs eagerly, like before.

    ``step(batch, actual_energy, actual_force) -> loss`` (a clone of the graph's static scalar)."""

    use_graph = property(lambda self: self.enabled, lambda self, on: setattr(self, "enabled", on))

    def __init__(self, model, head, model_3d="schnet", lr=5e-4, weight_decay=0.0, energy_coeff=0.05, force_coeff=0.95,
                 loss="l1", use_graph=True, max_graphs=16):
        self.model, self.head, self.model_3d = model, head, model_3d
        self.coeff, self.loss_kind = (float(energy_coeff), float(force_coeff)), loss
        self.flat = FlatParams([model, head])
        self.opt = FusedAdam(self.flat, lr=lr, weight_decay=weight_decay)
        StructureGraphs.__init__(self, max_graphs, enabled=use_graph)

    # ---- the step as eager launches (what a capture records)
    def _body(self, x, positions, batch_vec, rei, y_e, y_f, ones):
        pos = positions.detach().requires_grad_(True)                                                   # :33
        if self.model_3d == "painn":
            rep = self.model(x, pos, rei, batch_vec)
        else:
            rep = self.model(x if x.dim() == 1 else x[:, 0], pos, batch_vec)   # (MD17 batches: 1-D x, datasets_MD17.py:61)
        energy = self.head(rep).squeeze(1)                                                              # :36-44
        dE = torch.autograd.grad(energy, pos, grad_outputs=ones, create_graph=True, retain_graph=True)[0]   # :46
        loss = ops.energy_force_loss(energy, y_e, dE, y_f, self.coeff[0], self.coeff[1], self.loss_kind)    # :46-51
        self.flat.zero_grad()
        with _lib.direct_grads():
            loss.backward(inputs=self.flat.trainable)                                                   # :53
        return loss.detach()

    def _key(self, batch_vec, rei, sizes, n_atoms):
        if self.model_3d == "painn":
            return tensors_key(batch_vec, rei)
        return tensors_key(batch_vec) if sizes is None else sizes_key(n_atoms, sizes)

    def _capture(self, batch, y_e, y_f):
        B = int(y_e.numel())
        dev = batch.positions.device
        bvec = batch.batch if self.model_3d == "painn" else owned_batch_vector(batch.batch)   # (PaiNN: the caller's own)
        st = dict(x=batch.x.clone(), pos=batch.positions.detach().clone(), y_e=y_e.detach().clone(),
                  y_f=y_f.detach().clone(), ones=torch.ones(B, dtype=torch.float32, device=dev),
                  bvec=bvec, rei=getattr(batch, "radius_edge_index", None) if self.model_3d == "painn" else None)
        run = lambda: self._body(st["x"], st["pos"], st["bvec"], st["rei"], st["y_e"], st["y_f"], st["ones"])
        warm_up(lambda: (run(), run()))   # (layouts, incidence lists, kernel attributes)
        with capture(self, "the force-training step", "enabled") as cap:
            st["graph"], st["loss"] = cap.record(run)
        if not cap.ok:
            return None
        self.flat.rebind_grads()
        return st

    def step(self, batch, actual_energy, actual_force):
        _lib.require_cuda(batch.positions, actual_energy, actual_force)
        if actual_energy.numel() != batch.num_graphs or tuple(actual_force.shape) != tuple(batch.positions.shape):
            raise ValueError("targets: one energy per molecule, one force row per atom")
        key = self._key(batch.batch, getattr(batch, "radius_edge_index", None), getattr(batch, "_sizes", None),
                        batch.batch.numel())
        hit = self.lookup(key, lambda: key[0] == "sizes", lambda: self._capture(batch, actual_energy, actual_force))
        if hit is None or hit[0]["x"].shape != batch.x.shape:   # (1-D against 2-D x: the key holds no x)
            ones = torch.ones(batch.num_graphs, dtype=torch.float32, device=batch.positions.device)
            loss = self._body(batch.x, batch.positions, batch.batch, getattr(batch, "radius_edge_index", None),
                              actual_energy, actual_force, ones)
            self.flat.rebind_grads()
        else:
            g = hit[0]   # (a new graph's inputs are copied in too: the step that captures is launched like every replay)
            copy_static([(g["x"], batch.x), (g["pos"], batch.positions), (g["y_e"], actual_energy.reshape(g["y_e"].shape)),
                         (g["y_f"], actual_force)])
            g["graph"].replay()   # (no _lib.poll_status behind it, deliberately for now: host work in a pinned step)
            loss = g["loss"].clone()
        self.opt.step()                                                                                 # :54
        return loss
