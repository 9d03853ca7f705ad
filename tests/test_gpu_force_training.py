"""Training on forces (examples/finetune_md17.py:31-54) against its fp64 twin (tests/force_twin.py): the loss, energies,
forces and the gradient of every backbone and head parameter of one step, per tensor max|got - ref| / max|ref| within
force_twin.BOUNDS, through three entry points - (a) the reference loop as written on the library's modules, with a
second step after a stock Adam update, (b) ForceTrainer launched eagerly, (c) ForceTrainer captured and replayed over
three steps - at the reference's MD17 configuration (SchNet 10 A, mean readout, 1-D x, L1 0.05 / 0.95, B = 1 / 128), on
the benchmark's workload, at the other fused widths, at the edges (1- and 2-atom molecules, a molecule without pairs, the
32-neighbour cap), for PaiNN past the tape's deferral limit, and under the switches of the second-order route.  The twin
runs in fp64 on the same device (torch's own kernels), cached per module."""
import hashlib
import json

import numpy as np
import pytest
import torch

import force_twin as tw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR = 5e-4
SCHNET_MD17 = dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                   readout="mean", node_class=9)
PAINN_MD17 = dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")
TWIN = {}       # content hash -> twin result (the twin of one step is shared by every entry point that takes it)
MEASURED = {}   # (case, entry) -> {quantity: worst error}


@pytest.fixture(scope="module", autouse=True)
def _lib_loaded():
    from geossl_amd import _lib
    _lib.load()
    yield
    print("\nFORCE_ERRORS " + json.dumps({"%s|%s" % k: v for k, v in sorted(MEASURED.items())}))


# --------------------------------------------------------------------------------------------------------------- cases
def _far_molecule(n, cutoff):
    """n atoms on a line, 1.5 cutoffs apart: no pair inside the cutoff."""
    return (np.arange(n, dtype=np.float32)[:, None] * np.float32(1.5 * cutoff) * np.array([[1, 0.3, 0.1]], np.float32))


def _raw(sizes, seed, cutoff, far=None):
    """make_batch over `sizes` (the first seed from `seed` on whose pairs all keep the twin's cutoff margin); molecule
    `far` (an index) gets positions without any pair inside the cutoff."""
    from geossl_amd.synthetic import make_batch
    for s in range(seed, seed + 50):
        r = make_batch(0, seed=s, sizes=sizes)
        if far is not None:
            off = int(np.sum(r["sizes"][:far]))
            r["positions"][off:off + sizes[far]] = _far_molecule(sizes[far], cutoff)
        if tw.cutoff_margin(r["positions"], r["batch"], cutoff) >= tw.CUTOFF_MARGIN:
            return r
    raise AssertionError("no seed with a cutoff margin")


def _moved(raw, k, cutoff):
    """raw with positions moved by up to ~0.05 A (step k of a replayed sequence), the cutoff margin kept."""
    g = np.random.default_rng(1000 + k)
    for _ in range(50):
        p = (raw["positions"] + 0.03 * g.standard_normal(raw["positions"].shape)).astype(np.float32)
        if tw.cutoff_margin(p, raw["batch"], cutoff) >= tw.CUTOFF_MARGIN:
            return dict(raw, positions=p)
    raise AssertionError("no move with a cutoff margin")


def _case(name):
    """name -> dict(kind, cfg, head, raw, x1d, loss, coeff, seed)."""
    from geossl_amd.synthetic import make_batch
    c = dict(kind="schnet", head="linear", x1d=False, loss="l1", coeff=(0.05, 0.95), seed=7)
    if name.startswith("schnet_md17_"):
        B, n = {"schnet_md17_B1": (1, 21), "schnet_md17_B128_n21": (128, 21), "schnet_md17_B128_n18": (128, 18)}[name]
        c.update(cfg=SCHNET_MD17, raw=_raw([n] * B, 11 + B + n, 10.0), x1d=True)
    elif name == "schnet_bench":   # bench.py force_training_line: 256 set-B molecules, seed 3, 5 A, add, Dense head, L1
        raw = make_batch(256, seed=3, mode="B")
        raw["x"][:, 0] = np.clip(raw["x"][:, 0], 1, 8)
        assert tw.cutoff_margin(raw["positions"], raw["batch"], 5.0) >= tw.CUTOFF_MARGIN
        c.update(cfg=dict(SCHNET_MD17, cutoff=5.0, readout="add"), raw=raw, head="dense")
    elif name == "schnet_F64_G64_L3":
        c.update(cfg=dict(hidden_channels=64, num_filters=64, num_interactions=3, num_gaussians=64, cutoff=5.0,
                          readout="mean", node_class=9), raw=_raw([9, 17, 3, 24, 12, 30], 31, 5.0))
    elif name == "schnet_F32_G8_L1":
        c.update(cfg=dict(hidden_channels=32, num_filters=32, num_interactions=1, num_gaussians=8, cutoff=5.0,
                          readout="add", node_class=9), raw=_raw([14, 2, 27, 8, 19], 32, 5.0), loss="mse",
                 coeff=(1.0, 10.0))
    elif name == "schnet_L12":
        c.update(cfg=dict(SCHNET_MD17, num_interactions=12, cutoff=5.0), raw=_raw([16, 11, 25, 4, 20], 33, 5.0))
    elif name == "schnet_edges":   # 1- and 2-atom molecules, one without pairs, 40 .. 255 atoms (the 32-neighbour cap)
        c.update(cfg=SCHNET_MD17, raw=_raw([1, 2, 5, 40, 1, 96, 255], 34, 10.0, far=2), x1d=True)
    elif name.startswith("painn_md17_"):
        c.update(kind="painn", head="painn", cfg=PAINN_MD17, x1d=True)
        if name == "painn_md17_B1":
            c["raw"] = _raw([21], 41, 5.0)
        elif name == "painn_md17_B128":
            c["raw"] = _raw([21] * 128, 42, 5.0)
        else:   # the smallest prefix of the B = 128 batch whose filter-network product exceeds the deferral limit
            c["raw"] = _painn_past_limit(_case("painn_md17_B128")["raw"])
    elif name.startswith("painn_"):
        F, R = {"painn_F128_R32": (128, 32), "painn_F64_R16": (64, 16), "painn_F32_R8": (32, 8),
                "painn_ragged_mean": (128, 20)}[name]
        sizes = [1, 12, 1, 7, 2, 19] if name == "painn_ragged_mean" else [13, 6, 22, 9]
        c.update(kind="painn", head="painn", cfg=dict(PAINN_MD17, n_atom_basis=F, n_rbf=R,
                                                      readout="mean" if name == "painn_ragged_mean" else "add"),
                 raw=_raw(sizes, 50 + F + R, 5.0))
    else:
        raise KeyError(name)
    return c


def _filter_product_bytes(E, cfg):
    """bytes of the operands of the filter network's weight gradient: [E, 3F L] against the radial basis [E, n_rbf
    padded to 8] (tape.painn_atom_features, `filters = linear(phi, ..)`)."""
    return 4 * E * (3 * cfg["n_atom_basis"] * cfg["n_interactions"] + -(-cfg["n_rbf"] // 8) * 8)


def _painn_past_limit(raw):
    from geossl_amd import tape
    from geossl_amd.synthetic import collate_subset
    from oracle.graph import radius_graph_np
    per_mol = []
    off = np.concatenate([[0], np.cumsum(raw["sizes"])])
    for m in range(len(raw["sizes"])):
        per_mol.append(radius_graph_np(raw["positions"][off[m]:off[m + 1]], 5.0).shape[1])
    E = np.cumsum(per_mol)
    k = int(np.nonzero(_filter_product_bytes(E, PAINN_MD17) > tape._DEFER_MAX_BYTES)[0][0]) + 1
    assert k < len(per_mol), "B = 128 does not pass the deferral limit"
    return collate_subset(raw, np.arange(k))


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _case(name)
    return _CASES[name]


# ------------------------------------------------------------------------------------------------------------ plumbing
def _modules(c):
    """Backbone and head with torch's own initialisation under a fixed seed.  (Not filler.py's closed-form weights: at
    10 A those make the forces cancel to ~1e-5 of the energy's scale, and a max-relative comparison of fp32 forces and of
    the gradients through them would then measure that cancellation, not the kernels.)"""
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    from geossl_amd.Geom3D.models.painn import Dense
    torch.manual_seed(1234)
    if c["kind"] == "schnet":
        model = SchNet(**c["cfg"]).to(DEV)
        F = c["cfg"]["hidden_channels"]
        head = (torch.nn.Linear(F, 1) if c["head"] == "linear" else Dense(F, 1)).to(DEV)
    else:
        model = PaiNN(**c["cfg"]).to(DEV)
        head = model.create_output_layers().to(DEV)
    return model, head


def _x(c, raw):
    return raw["x"][:, 0].copy() if c["x1d"] else raw["x"]


def _twin_cfg(c):
    cfg = c["cfg"]
    if c["kind"] == "schnet":
        return dict(num_interactions=cfg["num_interactions"], cutoff=cfg["cutoff"], readout=cfg["readout"])
    return dict(n_atom_basis=cfg["n_atom_basis"], n_interactions=cfg["n_interactions"], cutoff=cfg["cutoff"],
                readout=cfg["readout"])


def _edges(c, raw, rei=None):
    if c["kind"] == "schnet":
        return tw.schnet_edges(raw["positions"], raw["batch"], c["cfg"]["cutoff"])
    return rei.detach().cpu()


def _digest(*ts):
    h = hashlib.sha1()
    for t_ in ts:
        for v in (t_.values() if isinstance(t_, dict) else [t_]):
            a = torch.as_tensor(v).detach().cpu().contiguous()
            h.update(str((a.dtype, tuple(a.shape))).encode())
            h.update(a.numpy().tobytes())
    return h.hexdigest()


def _snapshot(model, head):
    p, b = tw.module_tensors(model)
    return p, b, tw.module_tensors(head)[0]


def _targets(c, snap, raw, ei, seed):
    p, b, h = snap
    e, f = tw.predict(c["kind"], _twin_cfg(c), p, b, h, _x(c, raw), raw["positions"], raw["batch"], ei, device=DEV)
    return tw.targets_with_margin(e, f, seed)


def _twin(c, snap, raw, ei, y_e, y_f):
    p, b, h = snap
    key = _digest(p, h, raw["positions"], raw["x"], raw["batch"], ei, y_e, y_f, torch.tensor(c["coeff"]),
                  torch.tensor([c["loss"] == "l1"]))
    if key not in TWIN:
        TWIN[key] = tw.step(c["kind"], _twin_cfg(c), p, b, h, _x(c, raw), raw["positions"], raw["batch"], ei, y_e, y_f,
                            coeff=c["coeff"], loss=c["loss"], device=DEV)
    return TWIN[key]


def _check(name, entry, got, ref, expect_all=True):
    errs = tw.errors(got, ref)
    if expect_all:   # every parameter of backbone and head compared
        want = set(ref["grads"]) | {"head." + k for k in ref["head_grads"]}
        assert {k[5:] for k in errs if k.startswith("grad/")} == want
    worst = {}
    for k, e in errs.items():
        q = k.split("/")[0]
        if e >= worst.get(q, (0.0, ""))[0]:
            worst[q] = (e, k)
    MEASURED[(name, entry)] = worst
    bad = tw.flagged(errs, case(name)["kind"])
    assert not bad, (name, entry, bad)
    return errs


def _named_grads(model, head):
    out = {}
    seen = set()
    for prefix, m in (("", model), ("head.", head)):
        for n, p in m.named_parameters():
            if id(p) not in seen:
                seen.add(id(p))
                out[prefix + n] = p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)
    return out


def _flat_grads(tr, model, head):
    """ForceTrainer's flat gradient split back into {name: grad} (FlatParams: model's parameters, then the head's)."""
    out, off, seen = {}, 0, set()
    for prefix, m in (("", model), ("head.", head)):
        for n, p in m.named_parameters():
            if id(p) in seen or not p.requires_grad:
                continue
            seen.add(id(p))
            out[prefix + n] = tr.flat.grad[off:off + p.numel()].view_as(p).detach().clone()
            off += p.numel()
    assert off == tr.flat.numel
    return out


def _gpu_batch(c, raw, host_sizes=True):
    from geossl_amd import ops
    from geossl_amd import pretrain_GeoSSL as pg
    d = dict(raw, x=_x(c, raw))
    if host_sizes:
        bt = pg.Batch.from_numpy(d, DEV)
    else:   # the reference's batch format: tensors only, no host-side sizes
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        bt = pg.Batch(tt(d["x"]), tt(d["positions"]), tt(d["batch"]), None)
    if c["kind"] == "painn":
        bt.radius_edge_index = ops.radius_graph(bt.positions, c["cfg"]["cutoff"], bt.batch)
    return bt


# ---------------------------------------------------------------------------------------------------------- entry points
def reference_loop(name, steps=2):
    """(a) finetune_md17.py:31-54 as written, on the library's modules, stock torch.optim.Adam between the steps."""
    c = case(name)
    raw = c["raw"]
    model, head = _modules(c)
    opt = torch.optim.Adam([{"params": model.parameters(), "lr": LR}, {"params": head.parameters(), "lr": LR}], lr=LR,
                           weight_decay=0)
    bt = _gpu_batch(c, raw, host_sizes=False)
    rei = getattr(bt, "radius_edge_index", None)
    ei = _edges(c, raw, rei)
    crit = torch.nn.L1Loss() if c["loss"] == "l1" else torch.nn.MSELoss()
    for k in range(steps):
        snap = _snapshot(model, head)
        y = _targets(c, snap, raw, ei, c["seed"] + k)   # (around this step's predictions: the L1 signs stay decided)
        y_e, y_f = y[0].to(DEV), y[1].to(DEV)
        positions = bt.positions.clone()
        positions.requires_grad_()                                                                           # :33
        if c["kind"] == "schnet":
            rep = model(bt.x if bt.x.dim() == 1 else bt.x[:, 0], positions, bt.batch)                        # :36
        else:
            rep = model(bt.x, positions, rei, bt.batch)                                                      # :38
        pred_energy = head(rep).squeeze(1)                                                                   # :41
        pred_force = -torch.autograd.grad(outputs=pred_energy, inputs=positions, grad_outputs=torch.ones_like(pred_energy),
                                          create_graph=True, retain_graph=True)[0]                           # :46
        loss = c["coeff"][0] * crit(pred_energy, y_e) + c["coeff"][1] * crit(pred_force, y_f)                # :51
        opt.zero_grad()
        loss.backward()                                                                                      # :53
        got = dict(loss=loss.detach(), energy=pred_energy.detach(), force=pred_force.detach(),
                   grads=_named_grads(model, head))
        _check(name, "a%d" % k, got, _twin(c, snap, raw, ei, *y))
        opt.step()                                                                                           # :54


def trainer_step(name, tag="b"):
    """(b) ForceTrainer(use_graph=False): one step, its flat gradient against the twin at the parameters before it."""
    from geossl_amd.graphed import ForceTrainer
    c = case(name)
    raw = c["raw"]
    model, head = _modules(c)
    tr = ForceTrainer(model, head, model_3d=c["kind"], lr=LR, energy_coeff=c["coeff"][0], force_coeff=c["coeff"][1],
                      loss=c["loss"], use_graph=False)
    bt = _gpu_batch(c, raw)
    ei = _edges(c, raw, getattr(bt, "radius_edge_index", None))
    snap = _snapshot(model, head)
    y_e, y_f = _targets(c, snap, raw, ei, c["seed"])
    loss = tr.step(bt, y_e.to(DEV), y_f.to(DEV))
    got = dict(loss=loss, grads=_flat_grads(tr, model, head))
    return _check(name, tag, got, _twin(c, snap, raw, ei, y_e, y_f))


def graph_steps(name, host_sizes=True, steps=3):
    """(c) ForceTrainer(use_graph=True): `steps` steps on new positions and targets of one structure, each step's flat
    gradient against the twin at the parameters read back before it -> the layer-loop forms the captures took."""
    from geossl_amd import ops
    from geossl_amd.graphed import ForceTrainer
    c = case(name)
    model, head = _modules(c)
    tr = ForceTrainer(model, head, model_3d=c["kind"], lr=LR, energy_coeff=c["coeff"][0], force_coeff=c["coeff"][1],
                      loss=c["loss"], use_graph=True)
    forms, real = [], ops.layer_loop

    def spy(ops_list, layout, *a, **k):
        plan, _ = layout.loop_plan()
        r = real(ops_list, layout, *a, **k)
        forms.append("none" if not r else ("ragged" if plan is None else "uniform"))
        return r

    ops.layer_loop = spy
    try:
        bt = None
        for k in range(steps):
            raw = _moved(c["raw"], k, c["cfg"]["cutoff"])
            if bt is None or (host_sizes and c["kind"] == "schnet"):
                bt = _gpu_batch(c, raw, host_sizes)   # SchNet with host sizes: a new batch object per step (key: sizes)
            else:   # one batch object, positions overwritten in place (a graph keyed by tensor identity replays)
                bt.positions.copy_(torch.from_numpy(raw["positions"]).to(DEV))
            ei = _edges(c, raw, getattr(bt, "radius_edge_index", None))
            snap = _snapshot(model, head)
            y_e, y_f = _targets(c, snap, raw, ei, c["seed"] + 1 + k)
            loss = tr.step(bt, y_e.to(DEV), y_f.to(DEV))
            torch.cuda.synchronize()
            _check(name, "c%d%s" % (k, "" if host_sizes else "-ref"), dict(loss=loss, grads=_flat_grads(tr, model, head)),
                   _twin(c, snap, raw, ei, y_e, y_f))
    finally:
        ops.layer_loop = real
    assert tr.use_graph and tr.captures == 1 and len(tr.graphs) == 1
    return set(forms)


# --------------------------------------------------------------------------------------------------------------- tests
MD17_SCHNET = ["schnet_md17_B1", "schnet_md17_B128_n21", "schnet_md17_B128_n18"]
MD17_PAINN = ["painn_md17_B1", "painn_md17_B128", "painn_md17_past_limit"]
FULL_ENTRY = MD17_SCHNET + ["schnet_bench"] + MD17_PAINN
OTHERS = ["schnet_F64_G64_L3", "schnet_F32_G8_L1", "schnet_L12", "schnet_edges", "painn_F128_R32", "painn_F64_R16",
          "painn_F32_R8", "painn_ragged_mean"]


@pytest.mark.parametrize("name", FULL_ENTRY + OTHERS)
def test_reference_loop_vs_twin(name):
    reference_loop(name)


@pytest.mark.parametrize("name", FULL_ENTRY + OTHERS)
def test_force_trainer_eager_vs_twin(name):
    trainer_step(name)


# the layer-loop form a captured SchNet step of each MD17 case takes (ops.layer_loop).  Measured: the ragged loop in
# every case, with host sizes too - ForceTrainer builds no block plan before its capture (layout.loop_plan makes none
# inside one), so the uniform loop of an 18-atom batch is not taken; the results meet the same bounds either way
LOOP_FORMS = {(name, host): {"ragged"} for name in ("schnet_md17_B1", "schnet_md17_B128_n21", "schnet_md17_B128_n18")
              for host in (True, False)}


@pytest.mark.parametrize("name,host_sizes", sorted(LOOP_FORMS))
def test_force_trainer_graph_vs_twin_schnet_md17(name, host_sizes):
    assert graph_steps(name, host_sizes) == LOOP_FORMS[(name, host_sizes)]


@pytest.mark.parametrize("name", ["schnet_bench"] + MD17_PAINN)
def test_force_trainer_graph_vs_twin(name):
    graph_steps(name)


def test_edge_batch_takes_the_neighbour_cap():
    """schnet_edges: the 32-neighbour cap of radius_graph (schnet.py:91) removes pairs at 10 A, and one molecule has no
    pair at all - the twin (and so the GPU, which met its bounds on this batch) saw both."""
    from oracle.graph import radius_graph_np
    raw = case("schnet_edges")["raw"]
    capped = radius_graph_np(raw["positions"], 10.0, raw["batch"])
    free = radius_graph_np(raw["positions"], 10.0, raw["batch"], max_num_neighbors=10 ** 6)
    assert capped.shape[1] < free.shape[1]
    deg = np.bincount(capped[1], minlength=raw["positions"].shape[0])
    assert deg.max() in (32, 33)   # (33 hits scanned, the self hit among them or not)
    off = int(np.sum(raw["sizes"][:2]))
    assert not np.isin(np.arange(off, off + 5), capped).any()


def test_painn_past_limit_batch_defers_and_refuses(monkeypatch):
    """The smallest PaiNN MD17 batch whose filter-network weight gradient ([E, 3F L] against the radial basis) is too
    large to wait for its batch (tape._tn_deferrable): in its second pass some column GEMMs are deferred and the filter
    network's is refused for size, and the step still meets the bounds (deferred and immediate contributions meet)."""
    from geossl_amd import tape
    c = case("painn_md17_past_limit")
    B = len(c["raw"]["sizes"])
    answers, real = [], tape._tn_deferrable

    def spy(a, b):
        r = real(a, b)
        if tape._PENDING is not None:
            ta, tb = a.t, b.t
            answers.append((r, tuple(ta.shape), tuple(tb.shape), 4 * ta.size(0) * (ta.size(1) + tb.size(1))))
        return r

    monkeypatch.setattr(tape, "_tn_deferrable", spy)
    trainer_step("painn_md17_past_limit", "b-spy")
    refused = [a for a in answers if not a[0] and a[3] > tape._DEFER_MAX_BYTES]
    assert any(a[0] for a in answers) and refused
    width = 3 * PAINN_MD17["n_atom_basis"] * PAINN_MD17["n_interactions"]
    assert any(width in (a[1][1], a[2][1]) for a in refused), refused
    # the smallest such batch: one molecule fewer stays below the limit
    smaller = tw.schnet_edges(c["raw"]["positions"][:-21], c["raw"]["batch"][:-21], 5.0).shape[1]
    assert _filter_product_bytes(smaller, PAINN_MD17) <= tape._DEFER_MAX_BYTES, (B, smaller)


@pytest.mark.parametrize("name,env,value", [("schnet_edges", "GEOSSL_SECOND_ORDER", "torch"),
                                            ("painn_ragged_mean", "GEOSSL_SECOND_ORDER", "torch"),
                                            ("schnet_bench", "GEOSSL_TAPE_NO_DEFER", "1"),
                                            ("painn_md17_past_limit", "GEOSSL_TAPE_NO_DEFER", "1"),
                                            ("schnet_md17_B128_n21", "GEOSSL_ARITH_24BIT", "1")])
def test_switches_meet_the_same_bounds(name, env, value, monkeypatch):
    monkeypatch.setenv(env, value)
    trainer_step(name, "b:%s=%s" % (env, value))


@pytest.mark.parametrize("name", ["schnet_bench", "painn_md17_B128"])
def test_comparison_catches_a_dropped_weight_gradient_contribution(name, monkeypatch):
    """Teeth: every batched weight-gradient launch run with accumulate=False - a later round of a weight's sum then
    overwrites the earlier ones - must be flagged against the twin.  A test that expects the check to fail."""
    from geossl_amd import ops
    real, asked = ops.linear_wgrad, []

    def overwrite(problems, *a, **k):
        asked.append(bool(k.get("accumulate", False)))
        k["accumulate"] = False
        return real(problems, *a, **k)

    monkeypatch.setattr(ops, "linear_wgrad", overwrite)
    with pytest.raises(AssertionError) as e:
        trainer_step(name, "teeth")
    assert any(asked), "no accumulating weight-gradient round ran"
    assert "grad/" in str(e.value)
    MEASURED.pop((name, "teeth"), None)


# ------------------------------------------------------------------------------------------- 1-D x, the MD17 batch format
@pytest.mark.parametrize("use_graph", [False, True])
def test_force_trainer_takes_one_dimensional_x(use_graph):
    """DatasetMD17 stores x as a 1-D atom-type vector (datasets_MD17.py:61): ForceTrainer's SchNet step gives, bit for bit,
    what it gives with the 2-D form (x[:, 0] the same types)."""
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.graphed import ForceTrainer
    c = case("schnet_md17_B1")
    out = {}
    for dim in (1, 2):
        model, head = _modules(c)
        tr = ForceTrainer(model, head, lr=LR, use_graph=use_graph)
        losses = []
        for k in range(3):
            raw = _moved(c["raw"], k, 10.0)
            x = raw["x"][:, 0].copy() if dim == 1 else raw["x"]
            bt = pg.Batch.from_numpy(dict(raw, x=x), DEV)
            gen = torch.Generator().manual_seed(k)
            losses.append(tr.step(bt, torch.randn(1, generator=gen).to(DEV), torch.randn(21, 3, generator=gen).to(DEV)))
        torch.cuda.synchronize()
        out[dim] = (torch.stack(losses), tr.flat.flat.clone())
    assert torch.equal(out[1][0], out[2][0]) and torch.equal(out[1][1], out[2][1])


def test_graphed_forward_takes_one_dimensional_x():
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.graphed import GraphedForward
    c = case("schnet_md17_B128_n18")
    model, _ = _modules(c)
    raw, outs = c["raw"], {}
    for dim in (1, 2):
        gf = GraphedForward(model)
        x = raw["x"][:, 0].copy() if dim == 1 else raw["x"]
        outs[dim] = [gf(pg.Batch.from_numpy(dict(raw, x=x), DEV)).clone() for _ in range(2)]   # capture, replay
        assert gf.captures == 1
    assert all(torch.equal(a, outs[2][0]) for a in outs[1] + outs[2])
    # a graph captured on one form, handed the other (same sizes): no replay over a wrong-sized copy, the eager result
    mixed = gf(pg.Batch.from_numpy(dict(raw, x=raw["x"][:, 0].copy()), DEV))
    assert gf.captures == 1 and torch.allclose(mixed, outs[2][0], rtol=1e-5, atol=1e-5)


# ----------------------------------------------------------------------------------- the tape's deferred weight gradients
def test_deferred_sums_hold_their_value_or_raise():
    """One weight feeding four same-shape products under tape.deferred_tn(): its gradient (a sum formed by the batched
    launches over four rounds) against fp64 autograd, and every intermediate value read after the flush - each free
    product its own value, each part of a sum and each sum taken over by a larger one either its own value or an error,
    never None or the sum."""
    from geossl_amd import tape as tp
    g = torch.Generator().manual_seed(5)
    R, M, N = 300, 48, 40
    W = torch.randn(M, N, generator=g)
    xs = [torch.randn(R, N, generator=g) for _ in range(4)]
    gs = [torch.randn(R, M, generator=g) for _ in range(4)]
    made, real_tn, real_total = [], tp._Deferred.tn, tp._Deferred.total

    def tn(self, a, b, *r, **k):
        n = real_tn(self, a, b, *r, **k)
        made.append(("part", n, a.t.double().cpu().t() @ b.t.double().cpu()))
        return n

    def total(self, x, y):
        s = real_total(self, x, y)
        if s is not None:
            made.append(("sum", s, None))
        return s

    tp._Deferred.tn, tp._Deferred.total = tn, total
    try:
        with torch.no_grad():
            w = tp.leaf(W.to(DEV))
            outs = [tp.mm(tp.const(x.to(DEV)), w, "nt") for x in xs]
            with tp.deferred_tn():
                (dw,) = tp.grad(outs, [tp.const(gg.to(DEV)) for gg in gs], [w])
            got = dw.t.double().cpu()
    finally:
        tp._Deferred.tn, tp._Deferred.total = real_tn, real_total
    ref = sum(gg.double().t() @ x.double() for x, gg in zip(xs, gs))
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-5
    parts = [m for m in made if m[0] == "part"]
    sums = [m for m in made if m[0] == "sum"]
    assert len(parts) == 4 and len(sums) == 3 and sums[-1][1] is dw
    for i, (_, v, want) in enumerate(made):
        if v is dw:
            continue
        if want is None:   # a smaller sum: its parts are the products made before it
            k = sums.index(made[i]) + 2
            want = sum(p[2] for p in parts[:k])
        try:
            val = v.t
        except RuntimeError:
            continue
        assert val is not None
        assert float((val.double().cpu() - want).abs().max() / want.abs().max()) < 1e-5, i
