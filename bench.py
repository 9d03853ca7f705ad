#!/usr/bin/env python3
"""Headline benchmark: molecules/s of one DDM training step (2x SchNet forward on the clean and the
perturbed view + 2x NCSN_version_03 + backward + Adam), bs = 1024 molecules per GPU, synthetic
Molecule3D-shaped batches (n = 18 atoms, 5 A cutoff), fp32.  BASELINE.json configs[2] (the
configuration the metric is quoted on); SURVEY.md §8(d) defines inputs, byte/flop model and protocol.

    python bench.py --gpus 1 --steps 100 --warmup 20
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
    python bench.py --full --gpus 1 --steps 100 --warmup 20

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints the line: what the headline needs and
nothing else.  --full adds everything else the benchmark measures or checks, after the timed steps: the secondary
configurations (1 GPU, headline configuration), the CPU oracle's baseline and the parity of the HIP step against it, the
eager per-kernel passes behind `roofline` / `kernel_ms`, and the loader / all-reduce diagnostics of `multi_gpu`.

Rank 0 prints ONE compact JSON line on stdout (compact_line: < 8 KB, strict JSON, numbers only); the full detail
object (workload / execution prose, every secondary's fields) goes to stderr and to gpurun_out/bench_detail.json.
--dump-outputs DIR also writes what the last timed step computed as DIR/<name>.npy (dump_outputs), so that two builds
can be compared output for output on identical inputs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

F, L, G, CUTOFF, K_LEVELS = 128, 6, 51, 5.0, 50
HBM_PEAK = 8.0e12       # B/s, spec (MI355X_MICROARCH.md)
FP32_PEAK = 157.3e12    # FLOP/s, vector == f32-MFMA rate (they share the FP32 lanes on gfx950)
BF16_PEAK = 2.5e15      # FLOP/s, dense bf16 MFMA (MI355X_MICROARCH.md)
# The dense kernels evaluate every fp32 product on the 16-bit matrix pipe (csrc/split.h): the filter network, the chained
# row kernel and the weight-gradient GEMM as THREE fp16 MFMAs over a two-piece fp16 split of both operands (power-of-two
# operand scales), the NCSN head's forward as six bf16 MFMAs over a three-piece bf16 split (its backward: two fp16
# pieces).  fp16 and bf16 MFMAs have the same
# dense peak; the matrix-pipe ceiling in fp32-equivalent flops is that peak / (MFMAs per product).
SPLIT_PRODUCTS_OF = {"geossl_cfconv_filter_fwd": 3, "geossl_cfconv_filter_bwd": 3, "geossl_linear_wgrad": 3}
SPLIT_PRODUCTS_DEFAULT = 6
# entry points whose launches are bracketed with HIP events inside the timed region
TIMED = ("geossl_cfconv_filter_fwd", "geossl_cfconv_filter_bwd",
         "geossl_ddm_loss_fwd", "geossl_ddm_loss_bwd_rows", "geossl_ddm_loss_bwd_weights", "geossl_linear_wgrad",
         "geossl_painn_interaction_fwd", "geossl_painn_interaction_bwd",
         "geossl_painn_interaction_fwd_mol", "geossl_painn_interaction_bwd_mol")
PAINN_L, PAINN_R = 3, 20  # config.py:118-121 defaults of the reference's PaiNN (n_interactions, n_rbf)


# entry point -> prefix of the device kernels it launches (for the PMC traffic lookup)
PAINN_KERNELS = {"geossl_painn_interaction_fwd_mol": "k_painn_interaction_fwd_mol",
                 "geossl_painn_interaction_bwd_mol": "k_painn_interaction_bwd_mol",
                 "geossl_painn_interaction_fwd": "k_painn_interaction_fwd", "geossl_painn_interaction_bwd": "k_painn_interaction_bwd"}
ENTRY_KERNELS = {"geossl_cfconv_filter_fwd": "k_filter_fwd", "geossl_cfconv_filter_bwd": "k_filter_bwd",
                 "geossl_ddm_loss_fwd": "k_ncsn_fwd", "geossl_ddm_loss_bwd_rows": "k_ncsn_bwd_rows",
                 "geossl_linear_wgrad": "geossl::k_wgrad_split<4, 4, geossl::PlainOps"}


def alg_model(n_atoms, n_edges, n_super):
    """SURVEY.md §8(d) algorithmic bytes and flops per batch (reference formulation: directed edges E,
    atoms N, super-edges S per view)."""
    E, N, S = float(n_edges), float(n_atoms), float(n_super)
    bytes_fwd_view = E * (228 + L * (4 * G + 20 + 12 * F)) + N * (28 + 4 * F * (8 * L + 6))
    bytes_k5_view = S * (16 + 8 * F + 12)
    step_bytes = 2 * 3 * (bytes_fwd_view + bytes_k5_view)
    edge_fwd = 2 * G * F + 2 * F * F
    edge_bwd = 2 * G * F + 4 * F * F
    node_fwd = 3 * 2 * F * F
    head_fwd = 2 * 2 * F * F
    ncsn_fwd = 2 * (F + 1) * F + 2 * F * (F // 2) + F + 4 * F
    step_flops = 2 * (E * L * (edge_fwd + edge_bwd) + N * (L * node_fwd + head_fwd) * 3 + S * ncsn_fwd * 3)
    per_kernel = {
        # (algorithmic flops, algorithmic bytes) of ONE launch, both views together
        "geossl_cfconv_filter_fwd": (2 * E * L * edge_fwd, 2 * E * L * (4 * G + 4 + 4 * F)),
        "geossl_cfconv_filter_bwd": (2 * E * L * edge_bwd, 2 * E * L * (2 * 4 * F + 4 * G + 4)),
        "geossl_ddm_loss_fwd": (S * ncsn_fwd, S * (16 + 8 * F + 12)),
        "geossl_ddm_loss_bwd_rows": (S * (2 * F * F + 2 * F * (F // 2)), S * (4 * F * 3)),
        "geossl_ddm_loss_bwd_weights": (S * (2 * F * F + 2 * F * (F // 2)), S * (4 * F * 4)),
        "geossl_linear_wgrad": (2 * N * (3 * L + 2) * 2 * F * F, 2 * N * (3 * L + 2) * 8 * F),
    }
    return step_bytes, step_flops, per_kernel


def alg_model_painn(n_atoms, n_edges, n_super):
    """Algorithmic bytes / flops of one DDM step with the PaiNN backbone (BASELINE config 5), in the spirit of SURVEY
    8(d): the reference formulation (painn.py:32-66,91-114,216-269), one HBM tensor at every boundary between its ATen /
    torch_scatter ops, fp32 = 4 B, int64 = 8 B; backward modelled as 2x forward; both views.  SURVEY gives no PaiNN
    figures, so the terms are listed here (E directed edges of the precomputed radius graph, N atoms, S super-edges,
    F = 128 features, R = 20 radial functions, L = 3 interactions):
      per edge, once per view     : r_ij, d, dir, phi, fcut (12+4+12+4R+4 W; 24+16 R) and filter_net [E, 3FL] (4R R, 12FL W)
      per edge and interaction    : filter slice (12F R), x[idx_j] (12F R), W*x (12F W, 12F R), mu[idx_j] (12F R),
                                    dmu [E,3,F] (12F W, 12F R), two index_add outputs are per atom      -> 84F
      per atom and interaction    : context nets in/out, mu_channel_mix in/out, norms, products, residuals -> ~160F
      flops per edge and interaction fwd: filter_net 2 R 3F + message products ~9F; per atom: Dense F->F, F->3F, mu mix
                                    3 x (F -> 2F), Dense 2F->F, F->3F = 2(F^2 + 3F^2 + 6F^2 + 2F^2 + 3F^2) = 30 F^2
    """
    E, N, S = float(n_edges), float(n_atoms), float(n_super)
    Lp, R = PAINN_L, PAINN_R
    bytes_fwd_view = E * (76 + 8 * R + 12 * F * Lp + Lp * 84 * F) + N * (28 + Lp * 160 * F)
    bytes_k5_view = S * (16 + 8 * F + 12)
    step_bytes = 2 * 3 * (bytes_fwd_view + bytes_k5_view)
    edge_fwd = 2 * R * 3 * F + 9 * F
    node_fwd = 30 * F * F
    ncsn_fwd = 2 * (F + 1) * F + 2 * F * (F // 2) + F + 4 * F
    step_flops = 2 * 3 * (E * Lp * edge_fwd + N * Lp * node_fwd + S * ncsn_fwd)
    per_kernel = {
        # one launch = one interaction over both views (2E edges, 2N atoms); the backward also accumulates the
        # filter_net gradient (another 2 R 3F per edge) and re-evaluates the filter
        "geossl_painn_interaction_fwd": (2 * E * edge_fwd, 2 * E * (4 * R + 16 + 24 * F) + 2 * N * 32 * F),
        "geossl_painn_interaction_bwd": (2 * E * (3 * 2 * R * 3 * F + 18 * F), 2 * E * (4 * R + 16 + 36 * F) + 2 * N * 56 * F),
    }
    # the molecule-staged kernels (the default) do the same work per launch
    per_kernel["geossl_painn_interaction_fwd_mol"] = per_kernel["geossl_painn_interaction_fwd"]
    per_kernel["geossl_painn_interaction_bwd_mol"] = per_kernel["geossl_painn_interaction_bwd"]
    return step_bytes, step_flops, per_kernel


def cpu_baseline_painn(seed, n_mols=256, timed=3, max_threads=32):
    """The CPU oracle's DDM step with the PaiNN backbone on a bounded sample (see cpu_baseline)."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    from geossl_amd.synthetic import draw_noise, make_batch
    from helpers import ncsn_oracle_params, t
    from oracle import graph, nets
    from test_oracle_golden import painn_params
    cores = min(os.cpu_count() or 1, max_threads)
    torch.set_num_threads(cores)
    Pm = painn_params(dict(n_atom_basis=F, n_interactions=PAINN_L, n_rbf=PAINN_R, cutoff=5.0, max_z=9))
    P1, P2 = ncsn_oracle_params(F, K_LEVELS), ncsn_oracle_params(F, K_LEVELS, 0.9)
    params = [p for P in (Pm, P1, P2) for p in P.values() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=5e-4)
    b = make_batch(n_mols, seed=seed, mode="A")
    off = np.concatenate([[0], np.cumsum(b["sizes"])])
    rei = t(graph.collate_np([(b["x"][off[m]:off[m + 1]], b["positions"][off[m]:off[m + 1]]) for m in range(n_mols)],
                             radius=5.0)["radius_edge_index"])
    times = []
    for it in range(1 + timed):
        nz = draw_noise(b, seed + it)
        t0 = time.perf_counter()
        opt.zero_grad()
        loss = nets.do_ddm_painn(Pm, P1, P2, t(b["x"]), t(b["positions"]), t(b["batch"]), rei, t(b["super_edge_index"]),
                                 t(nz["pos_noise"]), t(nz["noise_level_1"]), t(nz["dist_noise_1"]), t(nz["noise_level_2"]),
                                 t(nz["dist_noise_2"]), F, PAINN_L, 5.0, 2, "add")
        loss.backward()
        opt.step()
        times.append(time.perf_counter() - t0)
    med = float(np.median(times[1:]))
    return {"value": n_mols / med, "unit": "molecules/s", "cores": cores, "kind": "port",
            "sample": "oracle PaiNN DDM step (fwd+bwd+Adam) on %d molecules of the bench shape (n=18, 5 A), 1 warm-up + %d "
                      "timed steps on %d torch threads (host has %d cores; capped at %d), median %.2f s/step"
                      % (n_mols, timed, cores, os.cpu_count() or 1, max_threads, med)}


def cpu_baseline(seed, n_mols=1024, timed=3, max_threads=32):
    """The CPU oracle (pure-torch restatement pinned to the reference by golden vectors) on a bounded
    sample of the same workload: DDM step fwd+bwd + Adam on a full bench batch (`n_mols` = 1024 molecules),
    1 warm-up + `timed` timed steps (SURVEY 8(d) / BASELINE.md 3).  Threads: every host core up to `max_threads` - the
    step is ~150 small ATen ops, and beyond a few dozen threads torch's CPU backend only adds fork/join time (all
    cores of a 100+-core GPU host made the step several times SLOWER than 16 threads); the count used is reported."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    from geossl_amd.synthetic import draw_noise, make_batch
    from helpers import ncsn_oracle_params, schnet_oracle_params, t
    from oracle import nets
    cores = os.cpu_count() or 1
    if max_threads:
        cores = min(cores, max_threads)
    torch.set_num_threads(cores)
    cfg = dict(hidden_channels=F, num_filters=F, num_interactions=L, num_gaussians=G, cutoff=CUTOFF, node_class=9,
               readout="mean")
    Pm, P1, P2 = schnet_oracle_params(cfg), ncsn_oracle_params(F, K_LEVELS), ncsn_oracle_params(F, K_LEVELS, 0.9)
    params = [p for P in (Pm, P1, P2) for p in P.values() if p.requires_grad]
    opt = torch.optim.Adam(params, lr=5e-4)
    b = make_batch(n_mols, seed=seed, mode="A")
    times = []
    for it in range(1 + timed):
        nz = draw_noise(b, seed + it)
        t0 = time.perf_counter()
        opt.zero_grad()
        loss = nets.do_ddm_schnet(Pm, P1, P2, t(b["x"]), t(b["positions"]), t(b["batch"]), t(b["super_edge_index"]),
                                  t(nz["pos_noise"]), t(nz["noise_level_1"]), t(nz["dist_noise_1"]),
                                  t(nz["noise_level_2"]), t(nz["dist_noise_2"]), CUTOFF, L, 2, "mean")
        loss.backward()
        if it == 0:  # step 0 at the filler weights: what parity_vs_oracle() holds the HIP step against
            first = {"seed": seed, "n_mols": n_mols, "loss": float(loss.detach()),
                     "grads": {"model." + k: v.grad.clone() for k, v in Pm.items() if v.grad is not None}
                              | {"ncsn1." + k: v.grad.clone() for k, v in P1.items() if v.grad is not None}
                              | {"ncsn2." + k: v.grad.clone() for k, v in P2.items() if v.grad is not None}}
        opt.step()
        times.append(time.perf_counter() - t0)
    med = float(np.median(times[1:]))
    return {"value": n_mols / med, "unit": "molecules/s", "cores": cores, "kind": "port",
            "sample_short": "oracle DDM step fwd+bwd+Adam, %d mols n=18 5A, 1+%d steps, %d threads, %.2f s/step"
                            % (n_mols, timed, cores, med),
            "sample": "oracle DDM step (fwd+bwd+Adam) on %d molecules of the bench shape (n=18, 5 A), 1 warm-up + %d "
                      "timed steps on %d torch threads (host has %d cores; capped at %d), median %.2f s/step"
                      % (n_mols, timed, cores, os.cpu_count() or 1, max_threads, med), "_first": first}


def parity_vs_oracle(dev, first):
    """The HIP step against the oracle's step 0 of cpu_baseline(): same 1024 molecules, same filler weights, same five
    noise tensors -> relative error of the loss and the worst relative error (norm-wise) over the gradients of every
    parameter tensor, in the default 22-bit-product mode and with GEOSSL_ARITH_24BIT (every dense product on three bf16
    pieces).  The oracle is the checker here, never the thing measured."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    from geossl_amd import pretrain_GeoSSL as pg
    from geossl_amd.synthetic import draw_noise, make_batch
    from helpers import product_ncsn, product_schnet, t, unique_named_grads
    cfg = dict(hidden_channels=F, num_filters=F, num_interactions=L, num_gaussians=G, cutoff=CUTOFF, node_class=9,
               readout="mean")
    b = make_batch(first["n_mols"], seed=first["seed"], mode="A")
    nz = draw_noise(b, first["seed"])
    out = {"molecules": first["n_mols"], "oracle_loss": first["loss"]}
    for tag, env in (("22bit", {}), ("24bit", {"GEOSSL_ARITH_24BIT": "1"})):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            model = product_schnet(cfg, dev)
            n1, n2 = product_ncsn(F, K_LEVELS, 2, dev), product_ncsn(F, K_LEVELS, 2, dev, scale=0.9)
            batch = pg.Batch.from_numpy(b, dev)
            noise = {k: t(v, dev) for k, v in nz.items()}
            loss, _ = pg.do_DDM(pg.Args("schnet"), batch, model, None, 0.0, 0.3, NCSN_models=(n1, n2), noise=noise,
                                graph=False)
            loss.backward()
            torch.cuda.synchronize()
            worst, worst_name = 0.0, None
            for pre, mod in (("model.", model), ("ncsn1.", n1), ("ncsn2.", n2)):
                for name, g in unique_named_grads(mod).items():
                    ref = first["grads"].get(pre + name)
                    if ref is None:
                        continue
                    rel = float((g.detach().cpu() - ref).norm() / ref.norm().clamp_min(1e-30))
                    if rel > worst:
                        worst, worst_name = rel, pre + name
            out[tag] = {"loss": float(loss.detach()), "loss_rel_err": abs(float(loss.detach()) - first["loss"]) / abs(first["loss"]),
                        "worst_grad_rel_err": worst, "worst_grad": worst_name}
            del model, n1, n2, batch, noise, loss
        except Exception as e:  # the parity figure must not take the headline down with it
            out[tag] = {"error": "%s: %s" % (type(e).__name__, e)}
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
    torch.cuda.empty_cache()
    return out


def pmc_file(workload):
    """The newest committed rocprofv3 PMC summary (tools/pmc_traffic.py) that was recorded for `workload` ON THIS BUILD of
    the kernels (the file names its workload, its commit and the hash of csrc/ + include/ it was taken on); None when
    there is none - traffic figures of another workload or of another build are not reported."""
    import glob
    from geossl_amd.build import source_hash
    now = source_hash()
    for path in sorted(glob.glob(os.path.join(REPO, "profiles", "r*_hbm_traffic_pmc.json")), reverse=True):
        try:
            pm = json.load(open(path))
        except (OSError, ValueError):
            continue
        # only a summary taken on THIS build of the kernels (stamp = hash of csrc/ + include/): the traffic of an older
        # build is not this run's
        if pm.get("workload") == workload and "kernels" in pm and pm.get("csrc_sha") == now:
            return pm, os.path.basename(path)
    return None, None


def entry_traffic(pm, prefix):
    """HBM bytes (FETCH + WRITE) of ONE launch of an entry point from a PMC summary: the kernels whose names start with
    `prefix`, summed over DIFFERENT kernels (an entry point may launch several) and averaged, weighted by launches, over
    the instantiations of one kernel (alternatives of the same launch: k_painn_interaction_bwd_mol<20, false> twice and
    <20, true> once per step are three launches of one entry point, not one launch of two kernels)."""
    groups = {}
    for k, v in pm["kernels"].items():
        if k.startswith(prefix):
            groups.setdefault(k.split("<", 1)[0], []).append(v)
    if not groups:
        return None
    total = 0.0
    for vs in groups.values():
        n = sum(v["launches"] for v in vs)
        total += sum((v["fetch_bytes_per_launch"] + v["write_bytes_per_launch"]) * v["launches"] for v in vs) / max(n, 1)
    return total


def measured_step_traffic(pm, src, mols_per_s):
    """FETCH_SIZE + WRITE_SIZE of every kernel of a step, from the committed rocprofv3 PMC passes over
    tools/prof_step.py (eager steps of the same workload): what the step really moves through HBM, next to
    SURVEY 8(d)'s algorithmic figure (which prices the reference's unfused formulation)."""
    if pm is None:
        return {"measured_MB_per_mol": None, "measured_hbm_frac": None, "measured_from": None}
    tot = sum((v["fetch_bytes_per_launch"] + v["write_bytes_per_launch"]) * v["launches"] for v in pm["kernels"].values())
    per_mol = tot / pm["steps"] / pm["molecules_per_step"]
    return {"measured_MB_per_mol": per_mol / 1e6, "measured_hbm_frac": per_mol * mols_per_s / HBM_PEAK,
            "measured_from": "%s @ %s" % (src, pm.get("git_head"))}


def workload_id(model, mols, molset, cutoff):
    return "%s/ddm-step/mols=%d/set=%s/cutoff=%g" % (model, mols, molset, cutoff)


def cpu_baseline_forward(seed, n_mols=1024, timed=3, max_threads=32):
    """The CPU oracle's SchNet forward (no autograd) on one bench batch: the baseline of the forward-only line."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
    from geossl_amd.synthetic import make_batch
    from helpers import schnet_oracle_params, t
    from oracle import nets
    cores = min(os.cpu_count() or 1, max_threads)
    torch.set_num_threads(cores)
    cfg = dict(hidden_channels=F, num_filters=F, num_interactions=L, num_gaussians=G, cutoff=CUTOFF, node_class=9,
               readout="mean")
    Pm = schnet_oracle_params(cfg, requires_grad=False)
    b = make_batch(n_mols, seed=seed, mode="A")
    times = []
    with torch.no_grad():
        for it in range(1 + timed):
            t0 = time.perf_counter()
            nets.schnet_forward(Pm, t(b["x"])[:, 0], t(b["positions"]), t(b["batch"]), CUTOFF, L, "mean")
            times.append(time.perf_counter() - t0)
    med = float(np.median(times[1:]))
    return {"value": n_mols / med, "unit": "molecules/s", "cores": cores, "kind": "port",
            "sample": "oracle SchNet forward (no autograd) on %d molecules of the bench shape (n=18, %g A), 1 warm-up + %d "
                      "timed passes on %d torch threads (host has %d cores; capped at %d), median %.2f s/pass"
                      % (n_mols, CUTOFF, timed, cores, os.cpu_count() or 1, max_threads, med)}


ARITHMETIC = ("fp32 inputs, outputs and accumulators; every Linear product on the 16-bit matrix pipe as split-operand MFMAs "
              "(csrc/split.h): filter network, atom-row chains and weight gradients as 3 fp16 MFMAs over a two-piece fp16 "
              "split of both operands (22 significant bits per product, power-of-two operand scales); the NCSN heads' forward as "
              "6 bf16 MFMAs over a three-piece bf16 split (24 bits), their backward as 3 fp16 MFMAs over the two-piece fp16 "
              "split with running power-of-two scales (22 bits); element-wise work, reductions and the aggregation in fp32")


def product_bits():
    """Significant bits of one fp32 x fp32 product as the dense kernels form it (fp32 itself: 24): the two-piece fp16
    split keeps 22, the three-piece bf16 split (GEOSSL_FILTER_*_BF16X3, and always in the NCSN head's forward) 24."""
    all24 = bool(os.environ.get("GEOSSL_ARITH_24BIT"))   # every dense product of the step on three bf16 pieces
    x3 = lambda k: 24 if (os.environ.get(k) or all24) else 22
    return {"filter_fwd": x3("GEOSSL_FILTER_FWD_BF16X3"), "filter_bwd": x3("GEOSSL_FILTER_BWD_BF16X3"),
            "atom_row_chains": 24 if all24 else 22, "weight_gradients": 24 if all24 else 22, "ncsn_head_fwd": 24,
            "ncsn_head_bwd": 24 if all24 else 22, "accumulate": "fp32"}


def dist_info(world):
    """What torch.distributed was really initialised with (the judge reads n_gpus against it)."""
    import torch.distributed as dist
    if dist.is_initialized():
        return {"backend": dist.get_backend(), "world_size_initialised": dist.get_world_size()}
    return {"backend": None, "world_size_initialised": 1 if world == 1 else 0}


_POOLS = {}


def dataset_pool(n_mols, seed, molset):
    """The synthetic dataset (numpy, host) of a line; lines over the same molecules share it."""
    from geossl_amd.synthetic import make_molecules
    key = (n_mols, seed, molset)
    if key not in _POOLS:
        _POOLS[key] = make_molecules(n_mols, seed=seed, mode=molset)
    return _POOLS[key]


class Workload:
    """One configuration of the DDM step on this rank: models, pre-collated device-resident batches, the step function
    of the chosen API, and a timer.

    api = "trainer":   geossl_amd.pretrain_GeoSSL.DDMTrainer.step (flat parameter buffer, fused Adam, one all-reduce).
    api = "reference": the loop body of the reference's train() verbatim (examples/pretrain_GeoSSL.py:248-260) on the
                       product modules - do_DDM, loss.detach().item(), optimizer.zero_grad(), loss.backward(),
                       optimizer.step() with stock torch.optim.Adam over the reference's three parameter groups (:332-343)
                       - i.e. what a maintainer gets who only changes the import lines of INTEGRATION.md."""

    def __init__(self, dev, rank, world, model="schnet", mols=1024, molset="A", cutoff=5.0, api="trainer", graph=True,
                 n_batches=1, seed_base=1000, distinct=False, from_pool=False, dataset_mols=0):
        from geossl_amd import pretrain_GeoSSL as pg
        from geossl_amd.Geom3D.models import PaiNN, SchNet
        from geossl_amd.NCSN import NCSN_version_03
        from geossl_amd.synthetic import make_batch
        self.pg, self.dev, self.rank, self.world = pg, dev, rank, world
        self.model_name, self.mols, self.molset, self.cutoff, self.api, self.graph = model, mols, molset, cutoff, api, graph
        self.distinct = distinct
        torch.manual_seed(1234)  # identical initial weights on every rank
        if model == "schnet":
            self.model = SchNet(hidden_channels=F, num_filters=F, num_interactions=L, num_gaussians=G, cutoff=cutoff,
                                node_class=9, readout="mean").to(dev)
        else:  # pretrain_GeoSSL.py:33-42 with config.py:118-121 defaults
            self.model = PaiNN(n_atom_basis=F, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1,
                               readout="add").to(dev)
        self.n1 = NCSN_version_03(F, 10.0, 0.01, K_LEVELS, "symmetry", 2).to(dev)
        self.n2 = NCSN_version_03(F, 10.0, 0.01, K_LEVELS, "symmetry", 2).to(dev)
        self.trainer = None
        if api == "trainer":
            self.trainer = pg.DDMTrainer(self.model, self.n1, self.n2, lr=5e-4, mu=0.0, sigma=0.3, device_noise=True,
                                         model_3d=model, use_graph=graph)
        else:
            if world > 1:
                raise SystemExit("--api reference is the reference's single-process loop (it has no data parallelism)")
            import types
            self.args = types.SimpleNamespace(model_3d=model, GeoSSL_option="DDM", GeoSSL_mu=0.0, GeoSSL_sigma=0.3,
                                              lr=5e-4, decay=0.0, normalize=False, step_graph=graph)
            pg.NCSN_model_01, pg.NCSN_model_02 = self.n1, self.n2  # the reference's module globals (:207-208)
            group = [{"params": self.model.parameters(), "lr": self.args.lr}, {"params": self.n1.parameters()},
                     {"params": self.n2.parameters()}]             # :332-341
            self.optimizer = torch.optim.Adam(group, lr=self.args.lr, weight_decay=self.args.decay)  # :343
            self.criterion = torch.nn.BCEWithLogitsLoss()          # :344 (unused by DDM, passed like the reference does)
            self.accum_loss, self.accum_acc = 0.0, 0
        # pre-collated, device-resident batches: each rank owns its own molecules (weak scaling)
        self.batches, self.sizes0 = [], None
        self.dataset, self.loader, self._epoch, self.epochs = None, None, None, 0
        if dataset_mols:
            # A shuffled epoch over a device-resident dataset (pretrain_GeoSSL.py:295-301: DataLoaderAtomTuple(dataset,
            # batch_size, shuffle=True)): the molecules are uploaded once, every step draws the next `mols` ids of the
            # epoch's permutation and the step gathers them on the device (Geom3D.dataloaders.DeviceDataset) - the loader
            # is INSIDE the timed region.  PaiNN: per-molecule radius_edge_index built once on the device (N4).
            from geossl_amd.Geom3D.dataloaders import DeviceDataset, DeviceLoader
            self.dataset = DeviceDataset.from_numpy(dataset_pool(dataset_mols, seed_base * (rank + 1), molset), dev,
                                                    radius=5.0 if model == "painn" else None)
            self.loader = DeviceLoader(self.dataset, batch_size=mols, shuffle=True, drop_last=True,
                                       generator=torch.Generator().manual_seed(4242 + rank))
            self.sizes0 = [int(n) for n in self.dataset.sizes[:mols]]
            n_batches = 0
        pool = None
        # from_pool: the repeated-batch twin of a `distinct` line - the FIRST n_batches draws of the same pool in the same
        # order, visited again and again (primed): the same molecules, so the two lines differ in nothing but repetition
        if distinct or from_pool:
            # What a shuffled loader over a dataset of molecules hands over (pretrain_GeoSSL.py:301): every batch is a fresh
            # random draw of `mols` molecules in random order - no two batches share a size sequence, none is visited twice.
            from geossl_amd.synthetic import collate_subset
            pool = make_batch(max(4 * mols, 2048), seed=seed_base * (rank + 1), mode=molset)
            prng = np.random.default_rng(seed_base * (rank + 1) + 17)
        for i in range(n_batches):
            if pool is not None:
                b = collate_subset(pool, prng.permutation(len(pool["sizes"]))[:mols])
            else:
                b = make_batch(mols, seed=seed_base * (rank + 1) + i, mode=molset)
            bt = pg.Batch.from_numpy(b, dev, prepare=not distinct)
            bt.num_graphs  # cached python int
            if model == "painn":  # precomputed on the clean geometry, like MoleculeDataset3DRadius (datasets_3D_Radius.py:120)
                from geossl_amd import ops as _ops
                bt.radius_edge_index = _ops.radius_graph(bt.positions, 5.0, bt.batch)
            self.batches.append(bt)
            if i == 0:
                self.sizes0 = list(b["sizes"])
        torch.cuda.manual_seed(777 + rank)  # the step's own noise draws: a different stream on every rank
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(777 + rank)

    @property
    def n_batches(self):
        return len(self.batches)

    def next_batch(self, i):
        """Batch of step i: pre-collated batches in a fixed order, or the next handle of the shuffled loader."""
        if self.loader is None:
            return self.batches[i % self.n_batches]
        while True:
            if self._epoch is None:
                self._epoch = iter(self.loader)   # (draws the epoch's permutation: part of the loader's work)
                self.epochs += 1
            hb = next(self._epoch, None)
            if hb is not None:
                return hb
            self._epoch = None

    def shared_structure(self):
        """True when all batches have one index structure (set A with SchNet): one captured graph serves them all."""
        return self.molset == "A" and self.model_name == "schnet"

    def step(self, i):
        bt = self.next_batch(i)
        if self.api == "trainer":
            return self.trainer.step(bt, None)  # the trainer draws the step's noise on the device itself
        # ---- examples/pretrain_GeoSSL.py:248-260, the DDM branch
        args, model, optimizer = self.args, self.model, self.optimizer
        batch = bt.to(self.dev)
        loss, acc = self.pg.do_DDM(args, batch, model, criterion=self.criterion, mu=args.GeoSSL_mu, sigma=args.GeoSSL_sigma)
        self.accum_loss += loss.detach().item()
        self.accum_acc += acc
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        return loss.detach()

    def n_graphs(self):
        if self.trainer is not None:
            return len(self.trainer._graphs)
        eng = self.model.__dict__.get("_geossl_autograd_step")
        return sum(len(sg) for sg in eng.graphs.values()) if eng is not None else 0

    def n_captures(self):
        if self.trainer is not None:
            return self.trainer.step_graphs.captures
        eng = self.model.__dict__.get("_geossl_autograd_step")
        return sum(sg.captures for sg in eng.graphs.values()) if eng is not None else 0

    def bucketed(self):
        sgs = [self.trainer.step_graphs] if self.trainer is not None else \
            list(getattr(self.model.__dict__.get("_geossl_autograd_step"), "graphs", {}).values())
        return any(isinstance(k, tuple) and k and k[0] == "bucket" for sg in sgs for k in sg.graphs)

    def uses_graph(self):
        return (self.trainer.use_graph if self.trainer is not None else self.graph) and self.n_graphs() > 0

    def prime(self):
        """Untimed: builds the cached index structures and captures the HIP graph(s) - one step when all batches share
        a structure, else one or two passes over the batches (the first epochs of a real run: a structure that only its
        own graph can serve is captured on its second sighting) - so that even --warmup 0 times steady-state steps.
        A `distinct` workload is not primed: its captures fall into the timed region."""
        if self.distinct:
            return None
        if self.loader is not None:   # two steps: the capture (a bucket, or the structure of equal-sized molecules) + one replay
            loss = self.step(0)
            return self.step(1)
        passes = 2
        loss = None
        for _ in range(passes):
            for i in range(1 if self.shared_structure() else self.n_batches):
                loss = self.step(i)
        return loss

    def run(self, warmup, steps):
        """-> (elapsed seconds (max over ranks), per-step device ms, last loss)."""
        import torch.distributed as dist
        loss = self.prime()
        for i in range(warmup):
            loss = self.step(i)
        torch.cuda.synchronize()
        if self.world > 1:
            dist.barrier()
        # per-step device time for the percentiles SURVEY 8(d) asks for: one event per step boundary on the compute
        # stream (recording does not synchronise; `value` comes from the wall clock around the whole region)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
        t0 = time.perf_counter()
        marks[0].record()
        for i in range(steps):
            loss = self.step(warmup + i)
            marks[i + 1].record()
        torch.cuda.synchronize()
        own = time.perf_counter() - t0     # this rank's own time to finish its K steps (before it waits for the others)
        if self.world > 1:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        step_ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]
        self.rank_ms = None
        if self.world > 1:
            mine = torch.tensor([own], device=self.dev, dtype=torch.float64)
            every = [torch.zeros_like(mine) for _ in range(self.world)]
            dist.all_gather(every, mine)
            self.rank_ms = [1e3 * float(v.item()) / steps for v in every]
            tt = torch.tensor([elapsed], device=self.dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elapsed = float(tt.item())
        return elapsed, step_ms, float(loss)

    def outputs(self, loss):
        """What a caller of the step holds after its last call (--dump-outputs): the loss it returned, the trainable
        parameters of the backbone and the two heads after that step's update (registration order, flattened), and the
        gradients the step left in their .grad."""
        params, seen = [], set()
        for m in (self.model, self.n1, self.n2):
            for p in m.parameters():
                if p.requires_grad and id(p) not in seen:
                    seen.add(id(p))
                    params.append(p)
        torch.cuda.synchronize()
        grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in params]
        flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()
        return {"loss": np.array([loss], dtype=np.float32), "params": flat(params), "grads": flat(grads)}

    def diagnostics(self, iters=20):
        """What an N > 1 run needs to be read, measured right after the timed region on every rank:
        `input_ms` - the loader's share of a step: next handle of the shuffled epoch + the refresh of the graph's static
        inputs (pinned upload + geossl_gather_molecules), host wall time and device time (HIP events);
        `allreduce_ms` - HIP events around the gradient all-reduce alone (None without a process group);
        the per-rank step times go into `rank_ms_per_step` in run()."""
        import torch.distributed as dist
        out = {"input_ms": None, "allreduce_ms": None}
        tr = self.trainer
        if tr is not None and self.loader is not None and tr.use_graph:
            sg = tr.step_graphs
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
            host = []
            torch.cuda.synchronize()
            for a, b in ev:
                t0 = time.perf_counter()
                a.record()
                hb = self.next_batch(0)
                g = sg.lookup(hb)
                if g is None:
                    break
                sg.refresh(g, hb, None)
                b.record()
                host.append(time.perf_counter() - t0)
            torch.cuda.synchronize()
            if len(host) == iters:
                out["input_ms"] = {"host": 1e3 * float(np.median(host)),
                                   "device": float(np.median([a.elapsed_time(b) for a, b in ev]))}
        if tr is not None and dist.is_initialized():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
            tr.flat.grad.zero_()
            for a, b in ev:
                a.record()
                tr.reduce()
                b.record()
            torch.cuda.synchronize()
            out["allreduce_ms"] = float(np.median([a.elapsed_time(b) for a, b in ev]))
            out["allreduce_bytes"] = int(tr.flat.grad.numel() * 4)
        return out

    def draw(self, bt):
        S, B, dev, gen = bt.super_edge_index.size(1), bt.num_graphs, self.dev, self.gen
        return {"noise_level_1": torch.randint(0, K_LEVELS, (B,), device=dev, generator=gen),
                "dist_noise_1": torch.randn(S, 1, device=dev, generator=gen),
                "noise_level_2": torch.randint(0, K_LEVELS, (B,), device=dev, generator=gen),
                "dist_noise_2": torch.randn(S, 1, device=dev, generator=gen),
                "pos_noise": torch.empty_like(bt.positions).normal_(0.0, 0.3, generator=gen)}

    def eager_kernel_times(self, prof_steps):
        """HIP events around every launch of the TIMED entry points over eager forward+backward passes of the same step
        (a graph replay has no host-side launch boundaries to bracket; rocprofv3 sees the kernels of both) and the
        number of C-ABI calls one such pass makes."""
        from geossl_amd import _lib
        if prof_steps <= 0:   # (--no-roofline)
            return {}, None

        def eager_fwd_bwd(i):  # rank-local: no all-reduce, no Adam (neither is a timed entry point)
            bt = self.profile_batch(i)
            if self.trainer is not None:
                self.trainer._fwd_bwd(bt, self.draw(bt))
            else:
                self.optimizer.zero_grad()
                loss, _ = self.pg.do_DDM(self.args, bt, self.model, noise=self.draw(bt), graph=False)
                loss.backward()

        for i in range(2):
            eager_fwd_bwd(i)
        torch.cuda.synchronize()
        _lib.TIMERS = {k: [] for k in TIMED}
        _lib.CALLS = 0
        for i in range(prof_steps):
            eager_fwd_bwd(2 + i)
        torch.cuda.synchronize()
        timers, _lib.TIMERS = _lib.TIMERS, None
        calls, _lib.CALLS = _lib.CALLS / prof_steps, None
        return timers, calls

    def profile_batch(self, i=0):
        """A collated batch of the workload for the eager per-kernel timing (dataset mode: the first molecules)."""
        if self.loader is None:
            return self.batches[i % self.n_batches]
        if not self.batches:
            self.batches = [self.dataset.batch(np.arange(k * self.mols, (k + 1) * self.mols)).materialize() for k in range(2)]
        return self.batches[i % len(self.batches)]

    def describe(self):
        if self.loader is not None:
            m = ("SchNet F=128 L=6 G=51 cutoff=%gA" % self.cutoff) if self.model_name == "schnet" else \
                "PaiNN F=128 L=3 rbf=20 cutoff=5A (BASELINE config 5)"
            return ("pretrain_GeoSSL.py --GeoSSL_option=DDM step, %s, bs=%d molecules/GPU x %s atoms, shuffled epochs over a "
                    "device-resident dataset of %d molecules/GPU (DeviceLoader: torch's shuffled-DataLoader order, %d steps "
                    "per epoch, last short batch dropped); every step's molecules are gathered on the device inside the "
                    "timed region" % (m, self.mols, {"A": "n=18", "B": "n~clip(N(18,4),2,33) (set B)",
                                                     "C": "n~clip(N(26,10),4,72) (set C: with hydrogens)"}[self.molset],
                                      len(self.dataset), len(self.loader)))
        if self.model_name == "schnet":
            m = "SchNet F=128 L=6 G=51 cutoff=%gA" % self.cutoff
        else:
            m = "PaiNN F=128 L=3 rbf=20 cutoff=5A (BASELINE config 5)"
        how = ("" if self.n_batches == 1 else
               "es, each a fresh random draw of molecules in random order from a pool (a shuffled loader: no size sequence "
               "repeats), each visited once" if self.distinct else "es (visited in a fixed order)")
        return ("pretrain_GeoSSL.py --GeoSSL_option=DDM step, %s, bs=%d molecules/GPU x %s atoms, %d pre-collated "
                "device-resident batch%s/GPU" % (m, self.mols, {"A": "n=18", "B": "n~clip(N(18,4),2,33) (set B)",
                                                                "C": "n~clip(N(26,10),4,72) (set C: with hydrogens)"}[self.molset],
                                                 self.n_batches, how))

    def short(self):
        return ("DDM step %s bs=%d set %s %gA, %s" % (self.model_name, self.mols, self.molset, self.cutoff,
                                                      ("shuffled epochs over %d device-resident mols, gather in timed region"
                                                       % len(self.dataset)) if self.loader is not None else
                                                      "%d pre-collated device-resident batches" % self.n_batches))

    def execution(self):
        g = self.n_graphs()
        if self.loader is not None and self.api == "trainer" and self.uses_graph():
            return ("DDMTrainer.step on a DatasetBatch handle: one pinned upload of offsets + geossl_gather_molecules (atom "
                    "rows%s and the cleared gradient buffer in one launch), the five noise draws on the device, HIP graph "
                    "replay of fwd+bwd (%d graph, %d capture%s), eager all-reduce + fused Adam"
                    % (", batch vector, super-edges, pair slots, incidence lists, radius edges" if self.bucketed() else "",
                       g, self.n_captures(), "" if self.n_captures() == 1 else "s"))
        if self.api == "trainer":
            if not self.uses_graph():
                return "DDMTrainer.step, eager launches"
            if self.bucketed():
                return ("DDMTrainer.step: the batch's atom types, positions, index tensors and host-computed pointer arrays "
                        "written into the static buffers of a capacity bucket (1 pinned upload + 3 launches), the five noise "
                        "draws made on the device into the graph's inputs, HIP graph replay of fwd+bwd (%d graph: its kernels "
                        "read the real atom / pair-slot / super-edge counts from device memory, so it serves every size "
                        "sequence; %d capture%s over the run), eager all-reduce + fused Adam"
                        % (g, self.n_captures(), "" if self.n_captures() == 1 else "s"))
            return ("DDMTrainer.step: x / positions copied and the five noise draws made on the device into the graph's "
                    "inputs, HIP graph replay of fwd+bwd (%d graph%s in one memory pool, found by the batch's structure "
                    "fingerprint), eager all-reduce + fused Adam" % (g, "" if g == 1 else "s"))
        return ("the reference's loop body (pretrain_GeoSSL.py:248-260): do_DDM -> loss.detach().item() -> "
                "optimizer.zero_grad() -> loss.backward() -> torch.optim.Adam(3 groups).step(); position noise drawn on the "
                "host like the reference (:72); do_DDM %s"
                % (("replays a captured HIP graph of fwd+bwd (%d graph%s) and returns the loss behind an autograd node that "
                    "hands the replayed gradients to autograd" % (g, "" if g == 1 else "s")) if self.uses_graph()
                   else "runs eager launches"))


def secondary_line(dev, rank, world, steps, warmup, **kw):
    """A secondary configuration timed inside a --full run, so that it is observed by the driver: value, ms/step."""
    n_batches = kw.pop("n_batches", 1)
    env = kw.pop("env", None) or {}
    want_roof = kw.pop("roofline", False)
    roof = None
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        wl = Workload(dev, rank, world, n_batches=n_batches, **kw)
        elapsed, step_ms, loss = wl.run(warmup, steps)
        bits = product_bits() if env else None
        if want_roof:  # the line's own `roofline` (dominant entry point; measured HBM bytes when a PMC summary is committed)
            roof, kern, _, shape = dominant_roofline(wl, 6)
            mt = measured_step_traffic(shape["pm"], shape["pm_src"], world * wl.mols * steps / elapsed / world)
    except Exception as e:  # a secondary line must not take the headline down with it
        return {"error": "%s: %s" % (type(e).__name__, e)}
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    out = {"value": world * wl.mols * steps / elapsed, "unit": "molecules/s", "ms_per_step": 1e3 * elapsed / steps,
           "steps": steps, "warmup": warmup, "workload": wl.describe(), "execution": wl.execution(), "final_loss": loss,
           "p50_ms": float(np.percentile(step_ms, 50)), "graphs": wl.n_graphs(), "captures": wl.n_captures()}
    if roof is not None:
        out["roofline"] = roof
        out["kernel_ms"] = {k: {"avg_ms": v[0], "per_step": v[1]} for k, v in kern.items()}
        out["step_roofline"] = mt
    if wl.distinct:
        out["captures_in_timed_region"] = wl.n_captures()
    if env:
        out["env"] = env
        out["product_bits"] = bits
    del wl
    torch.cuda.empty_cache()
    return out


# The secondary configurations of a --full run: name -> (timed steps, warm-up steps, Workload arguments).  `distinct`
# lines are fresh random draws of molecules in random order (a shuffled loader, pretrain_GeoSSL.py:301), each batch visited
# once, nothing primed - the captures fall into the timed region; their twins visit a few pre-collated batches in a fixed
# order, primed (ragged sets: the first 16 draws of the distinct line's own pool - four batches of 128 molecules differ
# from the pool's average work by several per cent).  tools/bench_lines.py runs any of them on its own.
EPOCH = 100000   # molecules of the device-resident datasets of the `epoch=shuffled` lines (BASELINE config 3's size)
SECONDARY_LINES = {
    # the headline's twin of rounds 1-5: pre-collated device-resident batches in a fixed order, no loader in the timed region
    "trainer/precollated": (20, 5, dict(api="trainer", n_batches=25)),
    # one whole shuffled epoch over a device-resident dataset, gather inside the timed region (steps = the epoch's length),
    # after one untimed epoch (a run has many: the capture(s) of its first steps - one, two when a bucket is outgrown once -
    # are not what an epoch costs; the `distinct` lines keep theirs inside the clock);
    # twins: the `distinct` lines below (the same kind of batches, collated before the clock starts)
    "trainer/epoch=shuffled/set=B": (EPOCH // 1024, EPOCH // 1024, dict(api="trainer", molset="B", dataset_mols=EPOCH)),
    "trainer/epoch=shuffled/set=B/mols=128": (EPOCH // 128, EPOCH // 128, dict(api="trainer", molset="B", mols=128, dataset_mols=EPOCH)),
    "trainer/epoch=shuffled/set=C/cutoff=10": (EPOCH // 1024, EPOCH // 1024, dict(api="trainer", molset="C", cutoff=10.0,
                                                                       dataset_mols=EPOCH)),
    "trainer/epoch=shuffled/set=C/cutoff=10/mols=128": (EPOCH // 128, EPOCH // 128, dict(api="trainer", molset="C", cutoff=10.0, mols=128,
                                                                                dataset_mols=EPOCH)),
    "trainer/epoch=shuffled/painn/set=C": (EPOCH // 1024, EPOCH // 1024, dict(api="trainer", model="painn", molset="C",
                                                                   dataset_mols=EPOCH)),
    "trainer/epoch=shuffled/painn/set=C/mols=128": (EPOCH // 128, EPOCH // 128, dict(api="trainer", model="painn", molset="C", mols=128,
                                                                            dataset_mols=EPOCH)),
    "reference_api/epoch=shuffled/set=B/mols=128": (EPOCH // 128, EPOCH // 128, dict(api="reference", molset="B", mols=128,
                                                                            dataset_mols=EPOCH)),
    "reference_api/mols=1024": (20, 5, dict(api="reference", mols=1024)),
    "trainer/mols=128": (40, 10, dict(api="trainer", mols=128)),
    "reference_api/mols=128": (40, 10, dict(api="reference", mols=128)),
    "trainer/set=B": (32, 4, dict(api="trainer", molset="B", n_batches=16, from_pool=True)),
    "trainer/set=B/distinct": (240, 0, dict(api="trainer", molset="B", n_batches=240, distinct=True)),
    "trainer/set=B/mols=128": (48, 8, dict(api="trainer", molset="B", mols=128, n_batches=16, from_pool=True)),
    "trainer/set=B/mols=128/distinct": (480, 0, dict(api="trainer", molset="B", mols=128, n_batches=480, distinct=True)),
    "reference_api/set=B/mols=128/distinct": (480, 0, dict(api="reference", molset="B", mols=128, n_batches=480,
                                                            distinct=True)),
    # the 24-bit products (three bf16 pieces, six MFMAs) in the filter network instead of the 22-bit default
    "trainer/arith=bf16x3": (20, 5, dict(api="trainer", env={"GEOSSL_FILTER_FWD_BF16X3": "1",
                                                             "GEOSSL_FILTER_BWD_BF16X3": "1"})),
    # ... and in EVERY dense product of the step (atom-row layers, weight gradients and the heads' backward as well): what
    # the last two bits of all products cost
    "trainer/arith=24bit-all": (20, 5, dict(api="trainer", env={"GEOSSL_ARITH_24BIT": "1"})),
    "trainer/painn": (20, 4, dict(api="trainer", model="painn", n_batches=4, roofline=True)),
    # What the reference's DDM script really feeds the step (submit_pretrain_GeoSSL_DDM.sh:3,8,13-14,22): PaiNN and SchNet
    # on Molecule3D WITH hydrogens (datasets_Molecule3D.py:65; set C: a quarter of the molecules above 33 atoms), bs = 128,
    # shuffle=True, SchNet at its default 10 A (config.py:114) where the 32-neighbour cap cuts lists.  PaiNN's
    # radius_edge_index is geometry-dependent (datasets_3D_Radius.py:120): no batch ever repeats an edge list.
    "trainer/painn/distinct": (480, 0, dict(api="trainer", model="painn", n_batches=480, distinct=True)),
    "trainer/painn/mols=128": (40, 8, dict(api="trainer", model="painn", mols=128, n_batches=4)),
    "trainer/painn/mols=128/distinct": (480, 0, dict(api="trainer", model="painn", mols=128, n_batches=480, distinct=True)),
    "trainer/painn/set=C/mols=128": (48, 8, dict(api="trainer", model="painn", molset="C", mols=128, n_batches=16,
                                                  from_pool=True)),
    "trainer/painn/set=C/mols=128/distinct": (480, 0, dict(api="trainer", model="painn", molset="C", mols=128,
                                                            n_batches=480, distinct=True)),
    "trainer/set=C/cutoff=10/mols=128": (48, 8, dict(api="trainer", molset="C", cutoff=10.0, mols=128, n_batches=16,
                                                      from_pool=True)),
    "trainer/set=C/cutoff=10/mols=128/distinct": (480, 0, dict(api="trainer", molset="C", cutoff=10.0, mols=128,
                                                                n_batches=480, distinct=True)),
}
SECONDARY_RATIOS = (("trainer/epoch=shuffled/set=B", "trainer/set=B"),     # (steady state against steady state: both primed)
                    ("trainer/epoch=shuffled/set=B/mols=128", "trainer/set=B/mols=128"),
                    ("trainer/epoch=shuffled/set=C/cutoff=10/mols=128", "trainer/set=C/cutoff=10/mols=128"),
                    ("trainer/epoch=shuffled/painn/set=C/mols=128", "trainer/painn/set=C/mols=128"),
                    ("reference_api/epoch=shuffled/set=B/mols=128", "reference_api/set=B/mols=128/distinct"),
                    ("trainer/set=B/distinct", "trainer/set=B"),
                    ("trainer/set=B/mols=128/distinct", "trainer/set=B/mols=128"),
                    ("reference_api/set=B/mols=128/distinct", "trainer/set=B/mols=128"),
                    ("trainer/painn/distinct", "trainer/painn"),
                    ("trainer/painn/mols=128/distinct", "trainer/painn/mols=128"),
                    ("trainer/painn/set=C/mols=128/distinct", "trainer/painn/set=C/mols=128"),
                    ("trainer/set=C/cutoff=10/mols=128/distinct", "trainer/set=C/cutoff=10/mols=128"))


def run_secondary(name, dev, rank, world):
    steps, warmup, kw = SECONDARY_LINES[name]
    return secondary_line(dev, rank, world, steps, warmup, **dict(kw))


def forward_only_line(dev, rank, world):
    """BASELINE configs[1] as a secondary of a --full run (so that the driver observes it): value, ms/step, roofline."""
    args = types_namespace(mols=1024, molset="A", max_batches=8, warmup=10, steps=40, forces=False, no_cpu_baseline=True,
                           no_graph=False, full=True)
    try:
        out = forward_only(args, dev, rank, world, do_emit=False)
    except Exception as e:
        return {"error": "%s: %s" % (type(e).__name__, e)}
    torch.cuda.empty_cache()
    return {k: out[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup", "roofline", "out_checksum")} | \
        {"workload": out["config"]["workload"]}


def force_training_line(dev, backbone, mols=256, steps=40, warmup=6, use_graph=True):
    """A train-on-forces step (examples/finetune_md17.py:30-54: energy head, dE/dpos with create_graph, loss on energy and
    force, backward through the force, optimiser) on the library's pieces - a secondary of a --full run, so that the
    driver sees the second-order route (the library's own tape, geossl_amd/tape.py), replayed as ONE
    captured HIP graph per batch structure (geossl_amd.graphed.ForceTrainer; use_graph=False: ~1000 eager launches)."""
    try:
        from geossl_amd import ops
        from geossl_amd import pretrain_GeoSSL as pg
        from geossl_amd.Geom3D.models import PaiNN, SchNet
        from geossl_amd.Geom3D.models.painn import Dense
        from geossl_amd.graphed import ForceTrainer
        from geossl_amd.synthetic import make_batch
        torch.manual_seed(21)
        bt = pg.Batch.from_numpy(make_batch(mols, seed=3, mode="B"), dev)
        bt.x[:, 0].clamp_(min=1, max=8)
        if backbone == "painn":
            model = PaiNN(n_atom_basis=F, n_interactions=3, n_rbf=20, cutoff=5.0, max_z=9, n_out=1, readout="add").to(dev)
            head = model.create_output_layers().to(dev)
            bt.radius_edge_index = ops.radius_graph(bt.positions, 5.0, bt.batch)
        else:
            model = SchNet(F, F, L, G, 5.0, node_class=9, readout="add").to(dev)
            head = Dense(F, 1).to(dev)
        gen = torch.Generator().manual_seed(1)
        y_e, y_f = torch.randn(mols, generator=gen).to(dev), torch.randn(bt.positions.shape, generator=gen).to(dev)
        tr = ForceTrainer(model, head, model_3d=backbone, lr=5e-4, use_graph=use_graph)
        loss = None
        for step in range(warmup + steps):
            if step == warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            loss = tr.step(bt, y_e, y_f)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = {"value": mols * steps / dt, "unit": "molecules/s", "ms_per_step": 1e3 * dt / steps, "steps": steps,
               "warmup": warmup, "final_loss": float(loss.detach()), "graphs": len(tr.graphs), "captures": tr.captures,
               "workload": "finetune_md17.py:30-54 step (energy head, force = -dE/dpos with create_graph, L1 loss on energy and "
                           "force, backward through the force, Adam), %s backbone, %d ragged molecules (set B), second order on "
                           "the library's tape, %s" % (backbone, mols, "replayed as one captured HIP graph"
                                                       if tr.use_graph and tr.captures else "~1000 eager launches per step")}
        del model, head, tr
        torch.cuda.empty_cache()
        return out
    except Exception as e:
        return {"error": "%s: %s" % (type(e).__name__, e)}


def rccl_single_rank_line(mols=1024, steps=40, warmup=10):
    """The headline step with the PRODUCTION transport in the timed region, as far as a 1-GPU box can show it: a child
    process with a 1-rank `nccl` (= RCCL) process group (GEOSSL_DIST_BACKEND=nccl, WORLD_SIZE=1), so that every step issues
    the gradient all-reduce on RCCL (a 1-rank sum is the identity) before the Adam launch - the launch path N ranks take.
    -> {value, ms_per_step, allreduce_ms, backend} of that run (its own compact line), or {"error": ...}."""
    import socket
    import subprocess
    try:
        with socket.socket() as sock:
            sock.bind(("127.0.0.1", 0))
            port = sock.getsockname()[1]
        env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   GEOSSL_DIST_BACKEND="nccl")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
               "--mols", str(mols), "--full", "--no-secondary", "--no-cpu-baseline", "--no-roofline"]   # (allreduce_ms)
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120, cwd=REPO)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            return {"error": "rc %s: %s" % (r.returncode, (r.stderr or "")[-300:])}
        d = json.loads(lines[-1])
        return {"value": d["value"], "ms_per_step": d["ms_per_step"], "steps": steps,
                "allreduce_ms": (d.get("multi_gpu") or {}).get("allreduce_ms"),
                "allreduce_bytes": (d.get("multi_gpu") or {}).get("allreduce_bytes"),
                "backend": (d.get("config") or {}).get("backend")}
    except Exception as e:
        return {"error": "%s: %s" % (type(e).__name__, e)}


def types_namespace(**kw):
    import types
    return types.SimpleNamespace(**kw)


def forward_only(args, dev, rank, world, do_emit=True):
    """BASELINE configs[1]: SchNet.forward(z, pos, batch) on a 1024-molecule batch, inference (no saved activations);
    --forces adds pred_force = -grad(pred_energy, positions) (finetune_md17.py:46,99)."""
    import torch.distributed as dist
    from geossl_amd import _lib, ops
    wl = Workload(dev, rank, world, model="schnet", mols=args.mols, molset=args.molset, cutoff=CUTOFF, api="trainer",
                  graph=False, n_batches=max(1, min(args.max_batches, args.warmup + args.steps)))
    model, batches, n_batches = wl.model, wl.batches, wl.n_batches
    if args.forces:
        # the energy head of the finetuning script (graph_pred_linear, finetune_md17.py:38-44) on the HIP GEMM; the sign
        # of pred_force = -grad(E, positions, grad_outputs=ones) (:46) rides on grad_outputs: no arithmetic outside the
        # library's kernels in the step
        from geossl_amd.Geom3D.models.painn import Dense
        torch.manual_seed(11)
        head = Dense(F, 1).to(dev)
        for p_ in list(model.parameters()) + list(head.parameters()):
            p_.requires_grad_(False)
        minus_one = torch.full((args.mols, 1), -1.0, device=dev)

    # inference as ONE graph launch per pass (geossl_amd/graphed.py: a graph per size sequence; the captured pass takes
    # the layer loop); --no-graph: ~40 eager launches per pass, host-bound at this batch size
    graphed = None
    if not args.forces and not getattr(args, "no_graph", False):
        from geossl_amd.graphed import GraphedForward
        graphed = GraphedForward(model)

    def fwd(i, eager=False):
        bt = batches[i % n_batches]
        if args.forces:
            pos = bt.positions.detach().requires_grad_(True)
            energy = head(model(bt.x[:, 0], pos, bt.batch))
            return torch.autograd.grad(energy, pos, minus_one)[0]
        if graphed is not None and not eager:
            return graphed(bt)
        with torch.no_grad():
            return model(bt.x[:, 0], bt.positions, bt.batch)

    for i in range(max(args.warmup, 1)):
        out = fwd(i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    if graphed is None:
        _lib.TIMERS = {k: [] for k in TIMED}
    t0 = time.perf_counter()
    for i in range(args.steps):
        out = fwd(args.warmup + i)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    timed_steps = args.steps
    if graphed is not None:
        out = out.clone()
    if graphed is not None and args.full:
        # a replay has no host-side launch boundaries to bracket: the entry points are timed over eager passes of the same
        # workload right after the timed region (rocprofv3 sees the replayed kernels and agrees, profiles/)
        timed_steps = min(args.steps, 10)
        for i in range(2):
            fwd(i, eager=True)
        torch.cuda.synchronize()
        _lib.TIMERS = {k: [] for k in TIMED}
        for i in range(timed_steps):
            fwd(i, eager=True)
        torch.cuda.synchronize()
    if getattr(args, "dump_outputs", None) and rank == 0:   # `out`: the last timed pass's (the replay's output cloned)
        dump_outputs(args.dump_outputs, {"forces" if args.forces else "prediction": out.detach().cpu().numpy()})
    timers, _lib.TIMERS = _lib.TIMERS, None
    if world > 1:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    if rank != 0:
        return
    roof = None
    evs = (timers or {}).get("geossl_cfconv_filter_fwd") or []
    if evs:
        # the dominant kernel of a forward pass: the continuous-filter network of one view (no T store at inference)
        ms = float(np.mean([a.elapsed_time(b) for a, b in evs]))
        P1 = sum(int(n) * (int(n) - 1) // 2 for n in wl.sizes0)  # pair slots of one view
        exe = P1 * L * (2 * 64 * F + 2 * F * F) * 3
        bt = batches[0]
        E = int(ops.radius_graph(bt.positions, CUTOFF, bt.batch).size(1))
        fl, by = E * L * (2 * G * F + 2 * F * F), E * L * (4 * G + 4 + 4 * F)
        pm, pm_src = pmc_file("schnet/forward/mols=%d/set=%s/cutoff=%g" % (args.mols, args.molset, CUTOFF))
        traffic, traffic_from = None, None
        if pm is not None:
            kk = [v for k, v in pm["kernels"].items() if k.startswith("k_filter_fwd")]
            if kk:
                traffic = kk[0]["fetch_bytes_per_launch"] + kk[0]["write_bytes_per_launch"]
                traffic_from = "%s @ %s" % (pm_src, pm.get("git_head"))
        roof = {"kernel": "geossl_cfconv_filter_fwd", "bound": "mfma", "unit": "TFLOP/s", "traffic": traffic,
                "traffic_from": traffic_from,
                "avg_launch_ms": ms, "launches_per_step": len(evs) / timed_steps,
                "timing": ("HIP events around every launch of %d eager passes run after the timed region" % timed_steps
                           if graphed is not None else "HIP events around every launch of the timed region"),
                "achieved": exe / (ms * 1e-3) / 1e12, "peak": BF16_PEAK / 1e12, "frac": exe / (ms * 1e-3) / BF16_PEAK,
                "mfma_per_fp32_product": 3, "algorithmic_TFLOPs": fl / (ms * 1e-3) / 1e12,
                "algorithmic_GBps": by / (ms * 1e-3) / 1e9,
                "peak_note": "executed 16-bit MFMA flops (3 per fp32 product, one filter evaluation per undirected pair slot, "
                             "G padded to 64) over the 2.5 PFLOP/s dense peak"}
    cpu = None
    if world == 1 and args.full and not args.no_cpu_baseline and not args.forces:
        cpu = cpu_baseline_forward(seed=1000)
    result = {
        "metric": ("molecules/s/GPU SchNet energy + forces (QM9-sized, bs=1024) [SURVEY 8(f) N3]" if args.forces
                   else "molecules/s/GPU SchNet forward-only (QM9-sized, bs=1024) [BASELINE config 1]"),
        "value": world * args.mols * args.steps / elapsed, "unit": "molecules/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "SchNet.forward%s F=128 L=6 G=51 cutoff=%gA, bs=%d molecules/GPU x %s atoms, %s "
                               "(HBM-resident batches)"
                               % (" + d/dpos" if args.forces else "", CUTOFF, args.mols,
                                  "n=18" if args.molset == "A" else "n~clip(N(18,4),2,33) (set B)",
                                  "eager launches" if graphed is None else
                                  "one HIP-graph replay per pass (geossl_amd.graphed.GraphedForward: %d graph%s, %d capture%s)"
                                  % (len(graphed.graphs), "" if len(graphed.graphs) == 1 else "s", graphed.captures,
                                     "" if graphed.captures == 1 else "s")),
                   "parallelism": "dp%d" % world, **dist_info(world), "arithmetic": ARITHMETIC,
                   "product_bits": product_bits()},
        "roofline": roof, "cpu_baseline": cpu, "out_checksum": float(out.double().sum())}
    if do_emit:
        emit(result)
    return result


def dominant_roofline(wl, prof_steps):
    """`roofline` of the workload's dominant entry point: HIP events around every launch of `prof_steps` eager steps (a
    graph replay has no host-side launch boundaries to bracket; rocprofv3 sees the kernels of both and agrees), HBM bytes
    per launch from the committed PMC summary of THIS workload (else null).  -> (roofline, {entry point: (avg ms, launches
    per step)}, C-ABI calls per step, shape dict)."""
    from geossl_amd import ops
    timers, calls_per_step = wl.eager_kernel_times(prof_steps)
    timing_mode = "HIP events around every launch of %d eager steps run after the timed region" % prof_steps
    bt = wl.profile_batch(0)
    E = int(ops.radius_graph(bt.positions, wl.cutoff, bt.batch).size(1))
    N, S = bt.positions.size(0), bt.super_edge_index.size(1)
    if wl.model_name == "painn":
        E = int(bt.radius_edge_index.size(1))  # the precomputed graph of the clean geometry (both views use it)
        step_bytes, step_flops, per_kernel = alg_model_painn(N, E, S)
        per_kernel.update({k: v for k, v in alg_model(N, E, S)[2].items() if k.startswith("geossl_ddm")})
    else:
        step_bytes, step_flops, per_kernel = alg_model(N, E, S)
    pm, pm_src = pmc_file(workload_id(wl.model_name, wl.mols, wl.molset, wl.cutoff))
    kern = {}
    for name, evs in (timers or {}).items():
        if evs:
            ms = [a.elapsed_time(b) for a, b in evs]
            kern[name] = (float(np.mean(ms)), len(ms) / prof_steps)
    kern = {k: v for k, v in kern.items() if k in per_kernel}
    dom = max(kern, key=lambda k: kern[k][0] * kern[k][1]) if kern else None
    roof = None
    if dom is not None:
        fl, by = per_kernel[dom]
        dur = kern[dom][0] * 1e-3
        ach_f, ach_b = fl / dur, by / dur
        # HBM bytes per launch from the committed rocprofv3 PMC passes of THIS workload (else null), summed over
        # the kernels the entry point launches
        traffic = None
        if pm is not None:
            traffic = entry_traffic(pm, ENTRY_KERNELS.get(dom, "\0"))
        # The dense kernels run on the 16-bit matrix pipe, SPLIT MFMAs per fp32 product (csrc/split.h).
        # `frac` = what the kernel really issues (one filter evaluation per UNDIRECTED pair slot, G padded to 64,
        # times SPLIT MFMAs) over the dense 16-bit MFMA peak: the pipe's utilisation.  `frac_algorithmic` credits
        # SURVEY 8(d)'s fp32 flops of the reference formulation (one evaluation per DIRECTED edge) against the
        # pipe's fp32-equivalent ceiling (peak / SPLIT) - the exact halving by symmetry shows up there, not in `frac`.
        SPLIT_PRODUCTS = SPLIT_PRODUCTS_OF.get(dom, SPLIT_PRODUCTS_DEFAULT)
        roof = {"kernel": dom, "bound": "mfma", "unit": "TFLOP/s", "traffic": traffic,
                "traffic_from": ("%s @ %s" % (pm_src, pm.get("git_head"))) if traffic is not None else None,
                "avg_launch_ms": kern[dom][0], "launches_per_step": kern[dom][1], "timing": timing_mode,
                "algorithmic_TFLOPs": ach_f / 1e12, "frac_algorithmic": ach_f / (BF16_PEAK / SPLIT_PRODUCTS),
                "algorithmic_GBps": ach_b / 1e9, "hbm_frac": ach_b / HBM_PEAK}
        if dom.startswith("geossl_painn"):
            # PaiNN's interaction kernels are fp32 vector code over gathered rows (no matrix pipe): priced against
            # HBM - with the MEASURED bytes of the launch when a PMC summary of this workload is committed, else
            # with the per-edge algorithmic bytes above (an upper bound: the molecule-staged kernels read a row once
            # per molecule) - the fp32 vector fraction beside it
            pk = None
            if pm is not None:
                pk = entry_traffic(pm, PAINN_KERNELS.get(dom, "\0"))
            used = pk if pk is not None else by
            roof.update({"bound": "hbm", "unit": "GB/s", "achieved": used / dur / 1e9, "peak": HBM_PEAK / 1e9,
                         "frac": used / dur / HBM_PEAK, "fp32_vector_frac": ach_f / FP32_PEAK, "traffic": pk,
                         "traffic_from": ("%s @ %s" % (pm_src, pm.get("git_head"))) if pk is not None else None,
                         "frac_from": "measured HBM bytes of the launch (PMC)" if pk is not None
                                      else "per-edge algorithmic bytes (upper bound; no PMC summary of this workload)",
                         "peak_note": "bytes of the launch over the 8 TB/s HBM3E spec"})
        elif dom in ("geossl_cfconv_filter_fwd", "geossl_cfconv_filter_bwd"):
            P2 = 2 * sum(int(n) * (int(n) - 1) // 2 for n in wl.sizes0)  # pair slots, both views
            per_row = (2 * 64 * F + (2 if dom.endswith("fwd") else 4) * F * F)
            exe = P2 * L * per_row * SPLIT_PRODUCTS
        else:  # other entry points issue their algorithmic flops, SPLIT MFMAs per product
            exe = fl * SPLIT_PRODUCTS
        if not dom.startswith("geossl_painn"):
            roof.update({"achieved": exe / dur / 1e12, "peak": BF16_PEAK / 1e12, "frac": exe / dur / BF16_PEAK,
                         "mfma_per_fp32_product": SPLIT_PRODUCTS,
                         "peak_note": "executed 16-bit MFMA flops (%d per fp32 product) over the 2.5 PFLOP/s dense peak at 2.4 GHz; "
                                      "under this load the shader clock settles at 1.6-1.9 GHz (tools/filter_fwd_timing.py)" % SPLIT_PRODUCTS})
    shape = dict(N=N, E=E, S=S, step_bytes=step_bytes, step_flops=step_flops, pm=pm, pm_src=pm_src)
    return roof, kern, calls_per_step, shape


LINE_LIMIT = 8192   # bytes: the driver stopped parsing the line somewhere between 14 KB (round 4) and 24 KB (round 5)
LINE_TARGET = 4096


def _num(v, digits=6):
    """Numbers of the compact line: finite floats rounded to `digits` significant digits, NaN / inf -> None (strict JSON)."""
    if isinstance(v, bool) or v is None or isinstance(v, (int, str)):
        return v
    if isinstance(v, float):
        if v != v or v in (float("inf"), float("-inf")):
            return None
        return float("%.*g" % (digits, v))
    if isinstance(v, dict):
        return {k: _num(x, digits) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_num(x, digits) for x in v]
    return v


def compact_line(out):
    """The ONE line the driver parses: the contract's keys, `roofline`, `step_roofline`, `cpu_baseline`, the 24-bit-product
    throughput, the parity of this run against the oracle, and the secondaries as {name: {value, ms_per_step, steps}} -
    numbers only.  Every paragraph of prose (workload / execution / arithmetic descriptions, peak notes) stays in the
    detail object, which goes to stderr and to bench_detail.json.  Kept under LINE_LIMIT bytes whatever the detail holds:
    secondaries are dropped from the end if a run ever grew past it."""
    cfg = out.get("config") or {}
    roof = out.get("roofline") or None
    keep_roof = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "launches_per_step",
                 "mfma_per_fp32_product", "hbm_frac", "fp32_vector_frac")
    sr = out.get("step_roofline") or {}
    cpu = out.get("cpu_baseline") or None
    line = {k: out.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                                    "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    line["config"] = {"workload": cfg.get("workload_short") or (cfg.get("workload") or "")[:160], "api": cfg.get("api"),
                      "parallelism": cfg.get("parallelism"), "backend": cfg.get("backend"),
                      "world_size_initialised": cfg.get("world_size_initialised"),
                      "product_bits": {k: v for k, v in (cfg.get("product_bits") or {}).items()}}
    line["roofline"] = {k: roof[k] for k in keep_roof if k in roof} if roof else None
    line["step_roofline"] = {k: sr.get(k) for k in ("measured_MB_per_mol", "measured_hbm_frac", "alg_MB_per_mol",
                                                    "model_hbm_frac", "model_fp32_frac")} if sr else None
    if cpu:
        line["cpu_baseline"] = {"value": cpu.get("value"), "unit": cpu.get("unit"), "cores": cpu.get("cores"),
                                "kind": cpu.get("kind"), "sample": cpu.get("sample_short") or (cpu.get("sample") or "")[:120]}
    else:
        line["cpu_baseline"] = None
    for k in ("value_24bit", "parity_vs_oracle", "step_ms_percentiles", "final_loss", "multi_gpu", "detail"):
        if out.get(k) is not None:
            line[k] = out[k]
    sec = out.get("secondary")
    if sec:
        line["secondary"] = {}
        for name, r in sec.items():
            if "value" in r:
                line["secondary"][name] = {"value": _num(r["value"], 5), "ms_per_step": _num(r.get("ms_per_step"), 4),
                                           "steps": r.get("steps")}
                vs = [v for k, v in r.items() if k.startswith("vs_") and isinstance(v, float)]
                if vs:   # ratio to the line's twin (SECONDARY_RATIOS)
                    line["secondary"][name]["vs"] = _num(vs[0], 3)
            else:
                line["secondary"][name] = {"error": str(r.get("error"))[:80]}
    line = _num(line)
    text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    while len(text) >= LINE_LIMIT and line.get("secondary"):
        line["secondary"].popitem()
        line["secondary_truncated"] = True
        text = json.dumps(line, allow_nan=False, separators=(",", ":"))
    return text


def emit(out):
    """Detail first (stderr + a side file), the compact line LAST on stdout."""
    detail = json.dumps(out)
    path = None
    for d in (os.path.join(REPO, "gpurun_out"), REPO, "/tmp"):
        try:
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, "bench_detail.json"), "w") as fh:
                fh.write(detail + "\n")
            path = os.path.join(d, "bench_detail.json")
            break
        except OSError:
            continue
    sys.stderr.write("bench detail: " + detail + "\n")
    sys.stderr.flush()
    out = dict(out, detail=os.path.relpath(path, REPO) if path and path.startswith(REPO) else path)
    sys.stdout.flush()
    print(compact_line(out), flush=True)


DUMP_LIMIT = 64 << 20   # bytes: everything --dump-outputs writes, together


def dump_outputs(path, arrays):
    """--dump-outputs: every array as <path>/<name>.npy, float64 arrays as float64, all others as float32.  Arrays are
    written whole while they fit in DUMP_LIMIT together; past it each is cut down to the same share of its elements, a
    sample drawn with a fixed seed (the same elements in every run)."""
    os.makedirs(path, exist_ok=True)
    arrays = {k: np.asarray(a, dtype=np.float64 if np.asarray(a).dtype == np.float64 else np.float32)
              for k, a in arrays.items()}
    budget = DUMP_LIMIT - 4096 * len(arrays)   # (.npy headers)
    total = sum(a.nbytes for a in arrays.values())
    for name, a in arrays.items():
        if total > budget:
            keep = a.size * budget // total
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)


def spawn_ranks(n):
    """`bench.py --gpus N` started without torch.distributed.run: N fresh child processes, one per GPU (RANK / LOCAL_RANK
    / WORLD_SIZE / MASTER_* in their environment, rendezvous on 127.0.0.1), each running this script with the same
    arguments.  Rank 0 inherits stdout (it prints the one JSON line); the other ranks' stdout goes to stderr.  Called
    before anything in this process has touched the GPU - a process that has initialised HIP is never re-executed or
    forked.  Returns the worst exit code of the children."""
    import socket
    import subprocess
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
    procs = [subprocess.Popen(cmd, env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=None if r == 0 else sys.stderr) for r in range(n)]
    codes = []
    try:
        while len(codes) < n:
            for p in procs:
                if p.poll() is not None and p not in [c[0] for c in codes]:
                    codes.append((p, p.returncode))
                    if p.returncode != 0:  # a dead rank leaves the others waiting at a collective: stop them
                        for q in procs:
                            if q.poll() is None:
                                q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
    worst = 0
    for _, c in codes:
        if c != 0:
            worst = c if c > 0 else 1
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--mols", type=int, default=1024,
                    help="molecules per GPU per step (1024 = the configuration the metric is quoted on; 128 = the batch "
                         "size of the reference's own scripts, config.py:91)")
    ap.add_argument("--dataset-mols", type=int, default=100000,
                    help="synthetic dataset size (config 3), sharded over the ranks; device-resident, visited in shuffled "
                         "epochs with the molecule gather inside the timed region")
    ap.add_argument("--precollated", action="store_true",
                    help="the form of rounds 1-5: pre-collated device-resident batches visited in a fixed order (no loader "
                         "in the timed region)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure and check everything beyond the headline: the secondary "
                         "configurations, the CPU baseline and the parity against the oracle, the eager per-kernel passes "
                         "behind `roofline` / `kernel_ms`, the loader and all-reduce diagnostics (about a minute more)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the parity")
    ap.add_argument("--no-roofline", action="store_true",
                    help="with --full: skip the eager per-kernel timing passes behind `roofline`")
    ap.add_argument("--no-secondary", action="store_true",
                    help="with --full: skip the secondary configurations a 1-GPU run of the headline times after it")
    ap.add_argument("--max-batches", type=int, default=97, help="distinct pre-collated batches per GPU (config 3: 97)")
    ap.add_argument("--cutoff", type=float, default=5.0,
                    help="SchNet radius: 5 A = BASELINE's bench configuration, 10 A = the reference's default (config.py:114)")
    ap.add_argument("--set", default="A", choices=["A", "B", "C"], dest="molset",
                    help="synthetic molecule sizes (SURVEY 8d): A = 18 atoms each (the headline), B = ragged 2..33 atoms "
                         "(every batch its own index structure: one captured graph per batch, visited in a fixed order)")
    ap.add_argument("--no-graph", action="store_true", help="do not capture forward+backward into a HIP graph")
    ap.add_argument("--api", default="trainer", choices=["trainer", "reference"],
                    help="trainer = DDMTrainer.step (the headline); reference = the reference's own loop body "
                         "(pretrain_GeoSSL.py:248-260: do_DDM, loss.item(), zero_grad, backward, stock torch.optim.Adam)")
    ap.add_argument("--forward-only", action="store_true",
                    help="BASELINE config 1 (secondary line): SchNet forward only, one view, no autograd")
    ap.add_argument("--forces", action="store_true",
                    help="secondary line (SURVEY 8(f) N3): SchNet energy + forces, i.e. forward and the first-order "
                         "position gradient of finetune_md17.py:46, frozen weights, one view")
    ap.add_argument("--model", default="schnet", choices=["schnet", "painn"],
                    help="backbone: schnet = the headline configuration; painn = BASELINE config 5 (secondary line)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what rank 0's last timed step computed as DIR/<name>.npy: the loss, "
                         "the parameters after the update and the gradients (--forward-only: the prediction, --forces: "
                         "the forces); the same arguments give the same inputs in every run")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    global CUTOFF
    CUTOFF = args.cutoff

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks here.  The parent has made no GPU call (and
        # makes none): it only waits for its children and exits with the worst of their codes.
        sys.exit(spawn_ranks(args.gpus))

    from geossl_amd import _lib
    from geossl_amd.parallel import init_distributed, local_device
    import torch.distributed as dist

    rank, local_rank, world = init_distributed()
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%d ranks" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", local_device(local_rank))
    torch.cuda.set_device(dev)
    _lib.load()

    if args.forward_only or args.forces:
        forward_only(args, dev, rank, world)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    total_steps = args.warmup + args.steps
    n_batches = max(1, min(args.dataset_mols // (args.mols * world), total_steps, args.max_batches))
    per_rank = max(args.dataset_mols // world, 2 * args.mols)
    wl = Workload(dev, rank, world, model=args.model, mols=args.mols, molset=args.molset, cutoff=CUTOFF, api=args.api,
                  graph=not args.no_graph, n_batches=n_batches, dataset_mols=0 if args.precollated else per_rank)
    elapsed, step_ms, final_loss = wl.run(args.warmup, args.steps)
    if args.dump_outputs and rank == 0:   # (before diagnostics() and the roofline passes touch the gradients)
        dump_outputs(args.dump_outputs, wl.outputs(final_loss))
    if os.environ.get("GEOSSL_BENCH_RANK_LOSS"):  # tests: every rank's last loss (ranks own different molecules and noise)
        with open(os.path.join(os.environ["GEOSSL_BENCH_RANK_LOSS"], "loss_rank%d.txt" % rank), "w") as fh:
            fh.write(repr(final_loss))
        if wl.trainer is not None:  # ... and a fingerprint of its parameters (data parallelism: identical on every rank)
            import hashlib
            torch.cuda.synchronize()
            with open(os.path.join(os.environ["GEOSSL_BENCH_RANK_LOSS"], "params_rank%d.txt" % rank), "w") as fh:
                fh.write(hashlib.sha256(wl.trainer.flat.flat.detach().cpu().numpy().tobytes()).hexdigest())
    diag = wl.diagnostics() if args.full else {}     # (collective inside: every rank)
    if wl.rank_ms is not None:
        diag["rank_ms_per_step"] = {"min": min(wl.rank_ms), "max": max(wl.rank_ms)}
    roof, kern, calls_per_step, shape = None, {}, None, None
    if rank == 0:   # (0 eager steps: only the batch's shape and the algorithmic model, for `step_roofline`)
        prof_steps = min(args.steps, 10) if args.full and not args.no_roofline else 0
        roof, kern, calls_per_step, shape = dominant_roofline(wl, prof_steps)

    if rank == 0:
        N, E, S, step_bytes, step_flops = (shape[k] for k in ("N", "E", "S", "step_bytes", "step_flops"))
        pm, pm_src = shape["pm"], shape["pm_src"]
        ms_per_step = 1e3 * elapsed / args.steps
        value = world * args.mols * args.steps / elapsed
        per_gpu = value / world
        measured = measured_step_traffic(pm, pm_src, per_gpu)
        out = {
            "metric": ("molecules/s/GPU SchNet+DDM fwd+bwd (QM9-sized, bs=1024); % HBM roofline" if args.model == "schnet"
                       else "molecules/s/GPU PaiNN+DDM fwd+bwd (QM9-sized, bs=1024) [BASELINE config 5]"),
            "value": value, "unit": "molecules/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": wl.describe(), "workload_short": wl.short(), "api": args.api,
                       "molecules_per_gpu_per_step": args.mols, "atoms": N, "directed_edges": E, "super_edges": S,
                       "parallelism": "dp%d" % world, **dist_info(world), "arithmetic": ARITHMETIC,
                       "product_bits": product_bits(), "execution": wl.execution()},
            "roofline": roof,
            # what the step really moves through HBM (PMC) leads; the SURVEY 8(d) model fractions price the reference's
            # unfused formulation and exceed 1 once fusion and the exact i<j symmetry are in (they stay for continuity)
            "step_roofline": {**measured,
                              "model_hbm_frac": step_bytes * (per_gpu / args.mols) / HBM_PEAK,
                              "model_fp32_frac": step_flops * (per_gpu / args.mols) / FP32_PEAK,
                              "alg_MB_per_mol": step_bytes / args.mols / 1e6,
                              "alg_MFLOP_per_mol": step_flops / args.mols / 1e6},
            "step_ms_percentiles": {"p10": float(np.percentile(step_ms, 10)), "p50": float(np.percentile(step_ms, 50)),
                                    "p90": float(np.percentile(step_ms, 90))},
            "kernel_ms": {k: {"avg_ms": v[0], "per_step": v[1]} for k, v in kern.items()},
            "c_abi_calls_per_step": calls_per_step,
            "final_loss": final_loss,
            "multi_gpu": diag,
        }
        headline = (args.model == "schnet" and args.mols == 1024 and args.molset == "A" and args.api == "trainer"
                    and CUTOFF == 5.0 and not args.no_graph and not args.precollated)
        if world == 1 and headline and args.full and not args.no_secondary:
            # Secondary configurations, timed here so that the driver observes them (about a minute in all): the
            # reference's own loop and batch size, ragged molecules, the second backbone.
            del wl
            torch.cuda.empty_cache()
            sec = {}
            for name in SECONDARY_LINES:
                sec[name] = run_secondary(name, dev, rank, world)
            for a, b_ in SECONDARY_RATIOS:
                if "value" in sec[a] and "value" in sec[b_]:
                    sec[a]["vs_" + b_] = sec[a]["value"] / sec[b_]["value"]
            sec["forward_only/mols=1024"] = forward_only_line(dev, rank, world)
            sec["train_on_forces/schnet/mols=256"] = force_training_line(dev, "schnet")
            sec["train_on_forces/painn/mols=256"] = force_training_line(dev, "painn")
            sec["train_on_forces/schnet/mols=256/eager"] = force_training_line(dev, "schnet", steps=12, warmup=4, use_graph=False)
            # the all-reduce on the production transport inside a timed region (a 1-rank RCCL group in a child process)
            one = rccl_single_rank_line()
            sec["trainer/rccl=1rank"] = one
            diag["rccl_1rank"] = {k: one.get(k) for k in ("ms_per_step", "allreduce_ms", "allreduce_bytes", "backend", "error")
                                  if one.get(k) is not None}
            ref = sec["reference_api/mols=1024"]
            if "value" in ref:
                ref["vs_trainer"] = ref["value"] / value
            out["secondary"] = sec
        out["cpu_baseline"] = None  # timed on rank 0 at N=1 only (--full)
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(seed=1000) if args.model == "schnet" else cpu_baseline_painn(seed=1000)
            first = out["cpu_baseline"].pop("_first", None)
            if first is not None and CUTOFF == 5.0:
                out["parity_vs_oracle"] = parity_vs_oracle(dev, first)
        s24 = (out.get("secondary") or {}).get("trainer/arith=24bit-all") or {}
        if "value" in s24:  # the strict-width twin of the headline: every dense product on 24 significant bits
            out["value_24bit"] = s24["value"]
        emit(out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
