"""CPU tests of the fp64 twin of training on forces (tests/force_twin.py): it reproduces fixtures G10, G13 and G22 (the
unmodified reference's finetune_md17.py:31-53 on CPU; G22 at the reference's own MD17 configuration, made by
tests/golden/make_golden_md17.py) within the tolerances of test_oracle_golden.py's G10 test, and the comparison the GPU
tests make with it flags a step that loses one atom's force residual."""
import json

import pytest
import torch

import force_twin as tw
from conftest import load_golden, rel_err
from helpers import fill_module_, grad_summary

G22 = ("schnet_B1", "schnet_B4", "painn_B1", "painn_B4")
TOL = 5e-5   # test_oracle_golden.py::test_g10_force_training_double_backward (the loss: 2e-5)


def _modules(kind, cfg, head_kind):
    from geossl_amd.Geom3D.models import PaiNN, SchNet
    if kind == "schnet":
        model = fill_module_(SchNet(**cfg))
        F = cfg["hidden_channels"]
    else:
        model = fill_module_(PaiNN(**cfg))
        F = cfg["n_atom_basis"]
    head = fill_module_(model.create_output_layers() if head_kind == "painn" else torch.nn.Linear(F, 1))
    return model, head


def _twin_of_fixture(g, kind, coeff, loss, **kw):
    cfg = json.loads(str(g["cfg"]))
    model, head = _modules(kind, cfg, kind)
    params, bufs = tw.module_tensors(model)
    hp, _ = tw.module_tensors(head)
    if kind == "schnet":
        ei = tw.schnet_edges(g["positions"], g["batch"], cfg["cutoff"])
        tcfg = dict(num_interactions=cfg["num_interactions"], cutoff=cfg["cutoff"], readout=cfg["readout"])
    else:
        ei = torch.from_numpy(g["radius_edge_index"])
        tcfg = dict(n_atom_basis=cfg["n_atom_basis"], n_interactions=cfg["n_interactions"],
                    cutoff=cfg["cutoff"], readout=cfg["readout"])
    return tw.step(kind, tcfg, params, bufs, hp, torch.from_numpy(g["x"]), torch.from_numpy(g["positions"]),
                   torch.from_numpy(g["batch"]), ei, torch.from_numpy(g["actual_energy"]),
                   torch.from_numpy(g["actual_force"]), coeff=coeff, loss=loss, **kw)


def _assert_reproduces(r, g):
    assert rel_err(r["loss"], g["loss"]) < 2e-5
    assert rel_err(r["energy"], g["energy"]) < TOL and rel_err(r["force"], g["force"]) < TOL
    assert rel_err(r["pos_grad"], g["grad_pos"]) < TOL
    for k in g:
        if k.startswith("head_grad/"):
            assert rel_err(r["head_grads"][k[10:]], g[k]) < TOL, k
        if k.startswith("gsum/"):
            assert rel_err(grad_summary(r["grads"][k[5:]]), g[k]) < TOL, k
        if k.startswith("grad/"):
            assert rel_err(r["grads"][k[5:]], g[k]) < TOL, k
    assert any(k.startswith("gsum/") for k in g)


@pytest.mark.parametrize("tag", ["reduced", "full_r5"])
def test_twin_reproduces_g10(tag):
    g = load_golden("g10_schnet_force_training_" + tag)
    _assert_reproduces(_twin_of_fixture(g, "schnet", (1.0, 10.0), "mse"), g)


def test_twin_reproduces_g13():
    g = load_golden("g13_painn_force_training")
    _assert_reproduces(_twin_of_fixture(g, "painn", (1.0, 10.0), "mse"), g)


@pytest.mark.parametrize("case", G22)
def test_twin_reproduces_g22(case):
    g = load_golden("g22_md17_" + case)
    meta = json.loads(str(g["meta"]))
    _assert_reproduces(_twin_of_fixture(g, meta["kind"], (meta["energy_coeff"], meta["force_coeff"]), "l1"), g)


def test_g22_cases_present():
    """The reference's MD17 configuration (config.py:111-115, finetune_md17.py:203-238): SchNet 128 / 128 / 6 / 51 at
    10 A with mean readout and PaiNN at its defaults, L1 with 0.05 / 0.95, 1-D x, one and four 21-atom molecules."""
    seen = set()
    for case in G22:
        g = load_golden("g22_md17_" + case)
        cfg, meta = json.loads(str(g["cfg"])), json.loads(str(g["meta"]))
        assert g["x"].ndim == 1 and g["positions"].shape == (21 * meta["B"], 3)
        assert (meta["loss"], meta["energy_coeff"], meta["force_coeff"]) == ("l1", 0.05, 0.95)
        if meta["kind"] == "schnet":
            assert cfg == dict(hidden_channels=128, num_filters=128, num_interactions=6, num_gaussians=51, cutoff=10.0,
                               readout="mean", node_class=9)
            assert set(k[10:] for k in g if k.startswith("head_grad/")) == {"weight", "bias"}
        else:
            assert cfg == dict(n_atom_basis=128, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add")
            assert set(k[10:] for k in g if k.startswith("head_grad/")) == {"0.weight", "0.bias", "1.weight", "1.bias"}
        seen.add((meta["kind"], meta["B"]))
    assert seen == {("schnet", 1), ("schnet", 4), ("painn", 1), ("painn", 4)}


def test_comparison_flags_one_dropped_force_residual():
    """The GPU tests' metric and bounds (force_twin.errors / BOUNDS): a step whose loss lost one atom's force residual -
    the size of the round-6 fault that dropped a term for a few atoms - is flagged; the twin against itself is not."""
    g = load_golden("g22_md17_schnet_B1")
    full = _twin_of_fixture(g, "schnet", (0.05, 0.95), "l1")
    again = _twin_of_fixture(g, "schnet", (0.05, 0.95), "l1")
    as_got = lambda r: dict(loss=r["loss"], energy=r["energy"], force=r["force"],
                            grads=dict(r["grads"], **{"head." + k: v for k, v in r["head_grads"].items()}))
    assert tw.flagged(tw.errors(as_got(again), full), "schnet") == {}
    dropped = _twin_of_fixture(g, "schnet", (0.05, 0.95), "l1", drop_force_atom=7)
    bad = tw.flagged(tw.errors(as_got(dropped), full), "schnet")
    assert any(k.startswith("grad/") for k in bad), bad


def test_twin_refuses_ambiguous_inputs():
    """A pair within 1e-4 A of the cutoff, or an L1 residual at zero: inputs on which fp32 and fp64 may differ."""
    pos = torch.tensor([[0.0, 0.0, 0.0], [5.00002, 0.0, 0.0], [0.0, 1.5, 0.0]])
    with pytest.raises(ValueError, match="cutoff"):
        tw.check_inputs(pos.numpy(), [0, 0, 0], 5.0)
    tw.check_inputs(pos.numpy(), [0, 1, 1], 5.0)   # (the near pair lies across two molecules)
    g = load_golden("g22_md17_schnet_B1")
    r = _twin_of_fixture(g, "schnet", (0.05, 0.95), "l1")
    g = dict(g, actual_force=r["force"].float().numpy().copy())
    g["actual_force"][0] += 1.0
    with pytest.raises(ValueError, match="L1"):
        _twin_of_fixture(g, "schnet", (0.05, 0.95), "l1")
