"""What ``md.Simulator`` and ``relax.Minimizer`` share: the molecules of a batch as B independent replicas on a force field.

``Replicas`` checks the batch (a collated batch with host sizes or a ``DeviceLoader`` handle; ragged sizes allowed), the
masses and the replay settings, and chooses the route.  The fused route - what ``predict_MD17`` serves on kernels alone
(``finetune_md17._fused_predict_ok``): SchNet up to 255 atoms, PaiNN on the interned complete pair list, the heads the
energy-head kernel takes - keeps the positions in a static device buffer that the force pass of
``finetune_md17._energy_and_gradient`` reads, with ``mol_ptr``, ``ACCEL / m`` and the graph owner beside it; a subclass adds
its own state in ``_alloc_fused`` and captures its step with ``_capture`` / ``_graph``.  The fallback route - CPU tensors, a
head or width the kernels do not serve, or an ``energy_and_gradient=callable(positions) -> (E [B], dE/dpos [N, 3])`` hook -
runs in torch operations in the dtype of the positions on ``md17_energy_force_aten(..., create_graph=False)``; a subclass
adds its state in ``_alloc_fallback``.  Refusals name the subclass."""
import types

import torch

from .finetune_md17 import (COMPLETE_MAX_N, _collated, _energy_and_gradient, _fused_predict_ok, complete_applies,
                            complete_edges, md17_energy_force_aten, with_complete_edges)
from .layout import get_layout
from .replay import StructureGraphs, capture, owned_batch_vector, parameter_addresses, warm_up

ACCEL = 4.184e-4                      # A fs^-2 per (kcal mol^-1 A^-1 amu^-1): 4184 J/kcal / (1e-3 kg/mol) * 1e-10 m/A * 1e-30
MAX_ATOMS = 255                       # per structure: the dense pair layout of the force pass
GRAPH_DEFAULT_MAX_ATOMS = 64 * 21     # use_graph None: replay up to this many atoms (measured for MD: md.py)


def default_masses(x):
    """MD17's encoding (datasets_MD17.py:56-59): x is the index into possible_atomic_num_list = [1..118], so the atom's
    mass is atomic_mass[x + 1] -> fp64 [N] on the CPU."""
    from .Geom3D.models._atomic_mass import atomic_masses
    table = torch.as_tensor(atomic_masses(), dtype=torch.float64).cpu()
    z = torch.as_tensor(x).detach().cpu().long()
    z = z if z.dim() == 1 else z[:, 0]
    if z.numel() and (int(z.min()) < 0 or int(z.max()) + 1 >= table.numel()):
        raise ValueError("default masses: atom types in [0, %d), got up to %d" % (table.numel() - 1, int(z.max())))
    return table[z + 1]


def _host_sizes(batch):
    sizes = getattr(batch, "_sizes", None)
    if sizes is None:
        sizes = torch.bincount(batch.batch.detach().cpu().long()).tolist()
    return [int(n) for n in sizes]


class Replicas:
    """See the module docstring.  A subclass calls ``_setup`` (checks; -> the collated batch), sets what its own state
    needs, then ``_route`` (-> ``fused``, the route's buffers, ``_alloc_fused(dev)`` or ``_alloc_fallback()``)."""

    def _setup(self, model, graph_pred_linear, batch, model_3d, masses, use_graph, steps_per_replay, max_frames,
               energy_and_gradient):
        who = type(self).__name__
        if model_3d not in ("schnet", "painn"):
            raise Exception("3D model {} not included.".format(model_3d))
        if int(steps_per_replay) < 1 or int(max_frames) < 1:
            raise ValueError("%s: steps_per_replay and max_frames are at least 1" % who)
        b = _collated(batch)
        self.model, self.head, self.model_3d = model, graph_pred_linear, model_3d
        self.hook = energy_and_gradient
        self.sizes = _host_sizes(b)
        self.B, self.N = len(self.sizes), int(b.positions.size(0))
        if sum(self.sizes) != self.N:
            raise ValueError("%s: the batch's sizes add up to %d atoms, positions has %d rows"
                             % (who, sum(self.sizes), self.N))
        if self.hook is None:
            if max(self.sizes) > MAX_ATOMS:
                raise ValueError("%s: structures of at most %d atoms (the dense pair layout of the force pass), "
                                 "got %d" % (who, MAX_ATOMS, max(self.sizes)))
            if model_3d == "painn" and (len(set(self.sizes)) != 1 or self.sizes[0] > COMPLETE_MAX_N):
                raise ValueError("%s: PaiNN runs on the interned complete pair list only (molecules of one size n "
                                 "<= %d); the radius edges of this batch would have to be rebuilt every step, which is "
                                 "not built" % (who, COMPLETE_MAX_N))
        m = default_masses(b.x) if masses is None else torch.as_tensor(masses).detach().cpu().double().reshape(-1)
        if m.numel() != self.N:
            raise ValueError("%s: masses has %d entries, the batch %d atoms" % (who, m.numel(), self.N))
        if not bool((m > 0).all()):
            raise ValueError("%s: masses are positive" % who)
        self.masses = m
        if use_graph is None:
            use_graph = self.N <= GRAPH_DEFAULT_MAX_ATOMS
        self.max_frames, self.steps_per_replay, self.use_graph = int(max_frames), int(steps_per_replay), bool(use_graph)
        self.graphs = None
        return b

    def _route(self, b):
        ps = None if self.hook is not None else _fused_predict_ok(self.model, self.head, b)
        if ps is not None and self.model_3d == "painn" and not complete_applies(types.SimpleNamespace(_sizes=self.sizes),
                                                                               self.model):
            ps = None   # (a subclass of PaiNN: the reference's lines on the complete pair list)
        self.fused = ps is not None and self._init_fused(ps, b)
        if not self.fused:
            self._init_fallback(b)

    # ---- the two routes' state
    def _init_fused(self, ps, b):
        dev = b.positions.device
        if self.model_3d == "painn":
            b = with_complete_edges(b, self.model)
            if not getattr(b, "_complete", False):   # (the switch is off: the reference's lines instead)
                return False
            bvec, rei = b.batch, b.radius_edge_index
        else:
            bvec, rei = owned_batch_vector(b.batch, self.sizes), None
        x = b.x.clone()
        self._x = x if self.model_3d == "painn" or x.dim() == 1 else x[:, 0].contiguous()
        self._ps, self._bvec, self._rei = ps, bvec, rei
        self._pos = b.positions.detach().clone().contiguous()
        if self._force() is None:   # (the backbone did not run as its fused node)
            return False
        f32 = dict(dtype=torch.float32, device=dev)
        self._vel = torch.zeros(self.N, 3, **f32)
        self._grad = torch.zeros(self.N, 3, **f32)
        self._energy = torch.zeros(self.B, **f32)
        self._cinv = (ACCEL / self.masses).to(**f32)
        self._mol_ptr = get_layout(bvec).mol_ptr
        self._alloc_fused(dev)
        self.graphs = StructureGraphs(4, enabled=self.use_graph)
        self._bound = parameter_addresses(self.model, self.head)
        return True

    def _init_fallback(self, b):
        pos = b.positions.detach().clone()
        dev, dt = pos.device, pos.dtype
        self._pos, self._vel = pos, torch.zeros_like(pos)
        self._x, self._bvec = b.x, b.batch
        self._rei = getattr(b, "radius_edge_index", None)
        if self.hook is None and self.model_3d == "painn":
            self._rei = complete_edges(self.B, self.sizes[0], dev)[0]
        self._cinv = (ACCEL / self.masses).to(device=dev, dtype=dt)[:, None]
        self._mol = torch.repeat_interleave(torch.arange(self.B), torch.tensor(self.sizes)).to(dev)
        self._grad = self._energy = None
        self._alloc_fallback()

    def _alloc_fused(self, dev):
        pass

    def _alloc_fallback(self):
        pass

    # ---- state
    @property
    def captures(self):
        return 0 if self.graphs is None else self.graphs.captures

    @property
    def positions(self):
        """The live positions [N, 3] (the force pass's static input on the fused route): clone to keep a copy."""
        return self._pos

    @property
    def velocities(self):
        return self._vel

    def set_positions(self, positions):
        self._pos.copy_(torch.as_tensor(positions).to(self._pos))

    # ---- the force pass
    def _force(self):
        return _energy_and_gradient(self.model_3d, self.model, self._ps, self._x, self._pos, self._bvec, self._rei)

    def _force_fallback(self):
        if self.hook is not None:
            energy, grad = self.hook(self._pos.detach())
            return energy.detach(), grad.detach()
        bd = types.SimpleNamespace(x=self._x, positions=self._pos.detach(), batch=self._bvec, radius_edge_index=self._rei)
        args = types.SimpleNamespace(model_3d=self.model_3d)
        with torch.enable_grad():
            energy, force = md17_energy_force_aten(args, bd, self.model, self.head, create_graph=False)
        return energy.detach(), force.detach().neg()

    # ---- capture
    def _capture(self, what, dry_run, body):
        """_Predictor._capture's protocol: the eager probe ran in _init_fused; warm-up passes that leave the state as it is
        (the force pass, SchNet's block plan, `dry_run()`: the subclass's kernels on copies); then `body()` into one graph."""
        def passes():
            self._force()
            if self.model_3d == "schnet":
                get_layout(self._bvec).loop_plan()
            dry_run()
        warm_up(passes)
        with capture(self.graphs, what, "enabled") as cap:
            graph, _ = cap.record(body)
        return dict(graph=graph) if cap.ok else None

    def _graph(self, key, make):
        """The captured graph under `key` (made by `make() -> entry or None` at first sight), or None: run eagerly."""
        if not self.use_graph:
            return None
        if self._bound != parameter_addresses(self.model, self.head):   # (parameters moved: the owner is rebuilt)
            self.graphs = StructureGraphs(4, enabled=self.graphs.enabled)
            self._bound = parameter_addresses(self.model, self.head)
        hit = self.graphs.lookup(key, lambda: True, make)
        return None if not hit else hit[0]["graph"]
