"""The fp64 twin of the NCSN head (tests/ncsn_twin.py) against autograd of the oracle, the conditioning of its inputs, and
the constant c of the GPU tests' bound |got - ref| <= c u S + A (tests/test_gpu_ncsn_backward.py)."""
import math

import pytest
import torch

import ncsn_twin as tw
from oracle import nets

U24 = 2.0 ** -24
QUANTITIES = ("dh",) + tw.KEYS


@pytest.mark.parametrize("K", [30, 50])
@pytest.mark.parametrize("power", [0.05, 2.0, 10.0])
def test_twin_gradients_equal_autograd_of_the_oracle(power, K):
    """dh and the ten parameter gradients written out by hand equal autograd of oracle.nets.ncsn_v03_forward in fp64 to
    1e-12 of each tensor's largest element: a ragged batch with a one-atom molecule in the middle and one at the end
    (the divisor of NCSN.py:210-212 is the last molecule WITH a super-edge), out_scale and an upstream scalar."""
    p = tw.ragged_problem([5, 1, 12, 2, 26, 3, 9, 1], 32, K, seed=7 + K)
    out_scale, upstream = 0.5, 3.0
    bw = tw.backward(p, power, out_scale=out_scale, upstream=upstream)
    P64 = {k: v.double().requires_grad_(k != "sigmas") for k, v in p["P"].items()}
    args = list(tw.oracle_args(p))
    args[2] = args[2].requires_grad_()
    (nets.ncsn_v03_forward(P64, *args, power) * out_scale * upstream).backward()
    want = {k: P64[k].grad for k in tw.KEYS}
    want["dh"] = args[2].grad
    for k in QUANTITIES:
        got = bw["g"][k].view_as(want[k])
        assert float((got - want[k]).abs().max()) <= 1e-12 * float(want[k].abs().max()), k
        assert bool((bw["S"][k].view_as(want[k]) >= got.abs() * (1 - 1e-12)).all()), k   # S bounds its own quantity
    one_atom = [5, 5 + 1 + 12 + 2 + 26 + 3 + 9]
    assert float(bw["g"]["dh"][one_atom].abs().max()) == 0.0 and float(bw["S"]["dh"][one_atom].abs().max()) == 0.0
    # the forward part is the function the packed-kernel test holds loss_e to
    loss, parts = nets.ncsn_v03_forward(P64, *args, power, return_parts=True)
    ref, S, _ = tw._ncsn_ref_and_bound(p, power)
    assert float((ref - parts["loss_e"].detach()).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert bool((S >= ref).all())


def test_row_margin_uses_propagated_magnitudes():
    """row_margin's denominator is M = |W| M_in + |b| through the layers: never above the |x| |W| of the actual
    activations (nets.ncsn_relu_margin), so a batch conditioned to T has at least T there."""
    p = tw.ragged_problem(tw.ragged_sizes(12, 5), 64, 30, seed=3)
    m = tw.row_margin(p)
    assert m.shape == (p["S"],) and bool((m >= 0).all())
    loose = nets.ncsn_relu_margin({k: v.double() for k, v in p["P"].items()}, *tw.oracle_args(p))
    assert float(m.min()) <= loose * (1 + 1e-12)


@pytest.mark.parametrize("name", sorted(tw.CASES))
def test_condition_is_reproducible_and_within_the_cap(name):
    """Every shape of the GPU file: `condition` gives the same problem from the same seed, removes at most 3 % of the
    rows, leaves no molecule without a super-edge it had, keeps the list grouped by molecule, and the oracle's own margin
    of the result is >= T."""
    q, S0, below, removed = tw.conditioned(name)
    assert removed <= tw.MAX_REMOVED * S0 and q["S"] == S0 - removed and below >= removed
    p = tw.CASES[name]()
    q2, below2, removed2 = tw.condition(p, generator=torch.Generator().manual_seed(tw.CONDITION_SEED))
    assert (below2, removed2) == (below, removed)
    for k in ("sei0", "sei1", "dist", "dn", "nl"):
        assert torch.equal(q[k], q2[k]), k
    e2g = q["batch"][q["sei0"]]
    assert bool((e2g[1:] >= e2g[:-1]).all()) and bool((q["batch"][q["sei1"]] == e2g).all())
    assert torch.equal(torch.unique(e2g), torch.unique(p["batch"][p["sei0"]]))
    assert float(tw.row_margin(q).min()) >= tw.T_MARGIN
    assert nets.ncsn_relu_margin({k: v.double() for k, v in q["P"].items()}, *tw.oracle_args(q)) >= tw.T_MARGIN
    # rows that were kept and never below T keep their noise
    kept = q2["kept"]
    same = (p["dn"][kept] == q["dn"]).view(-1)
    if torch.equal(p["nl"], q["nl"]):
        assert int((~same).sum()) <= below


@pytest.mark.parametrize("name", sorted(tw.PAIRS))
def test_condition_of_a_pair_of_heads(name):
    """Two heads on one super-edge list: each call of `condition` stays within the cap, both heads end on the same rows
    with margin >= T."""
    a, b, counts = tw.conditioned_pair(name)
    for rows, below, removed in counts:
        assert removed <= tw.MAX_REMOVED * rows
    assert torch.equal(a["sei0"], b["sei0"]) and torch.equal(a["sei1"], b["sei1"]) and a["S"] == b["S"]
    for q in (a, b):
        assert q["dist"].shape == (q["S"], 1) and q["dn"].shape == (q["S"], 1)
        assert float(tw.row_margin(q).min()) >= tw.T_MARGIN


def _r32(q, power, upstream=1.0):
    b64 = tw.backward(q, power, 0.5, upstream)
    b32 = tw.backward(q, power, 0.5, upstream, dtype=torch.float32)
    out = {}
    for k in QUANTITIES:
        S = b64["S"][k]
        err = (b32["g"][k].double() - b64["g"][k]).abs()
        assert bool((err[S == 0] == 0).all()), k
        out[k] = float((err / (U24 * S).clamp_min(1e-300)).max())
    return out


R32_CASES = [("ragged40-F32", 2.0, 1.0), ("ragged40-F64", 2.0, 1.0), ("ragged40-F128", 2.0, 1.0),
             ("one9-F128", 2.0, 1.0), ("one2-F128", 2.0, 1.0), ("ragged700-F128", 2.0, 1.0), ("bench", 2.0, 1.0),
             ("ragged300-F128", 0.05, 1.0), ("ragged300-F128", 2.0, 1e-9), ("ragged300-F128", 10.0, 1e6)]
_R32 = {}


@pytest.mark.parametrize("name,power,upstream", R32_CASES)
def test_fp32_evaluation_of_the_twin_stays_inside_the_bound(name, power, upstream):
    """The twin's expressions in torch.float32 (ATen: the reference's arithmetic) on the conditioned inputs: r32 = max
    |fp32 - fp64| / (2^-24 S) per quantity.  c = 4 max r32 (a different summation order over the rows, the dropped l l
    products), rounded up to a power of two, not below 8: the value ncsn_twin.C_BOUND must have."""
    r = _R32[(name, power, upstream)] = _r32(tw.conditioned(name)[0], power, upstream)
    print("r32 %s power %g upstream %g: %s" % (name, power, upstream, {k: round(v, 3) for k, v in r.items()}))
    c = max(8.0, 2.0 ** math.ceil(math.log2(max(4.0 * max(r.values()), 1e-30))))
    assert c <= tw.C_BOUND, (c, r)


def test_bound_constant_is_the_measured_one():
    """C_BOUND is exactly what the rule gives over the file's shapes (not a looser one)."""
    for case in R32_CASES:
        if case not in _R32:
            _R32[case] = _r32(tw.conditioned(case[0])[0], case[1], case[2])
    worst = max(max(r.values()) for r in _R32.values())
    assert tw.C_BOUND == max(8.0, 2.0 ** math.ceil(math.log2(max(4.0 * worst, 1e-30)))), worst


def test_absolute_term_is_negligible_at_power_two_and_not_at_the_ends():
    """A (the one-pass backward's operand scaling, ncsn_twin.absolute_term) against c u S with u = 2^-22: below 1/64 of
    it for every element at anneal_power 2, where the row gradients of all noise levels have one scale; at 0.05 and 10
    the atoms of low-noise molecules sit far below the running maximum and A is what bounds them."""
    q = tw.conditioned("ragged40-F128")[0]
    for power in (0.05, 2.0, 10.0):
        bw = tw.backward(q, power)
        A = tw.absolute_term(q, bw)
        worst = 0.0
        for k in QUANTITIES:
            S, a = bw["S"][k].reshape(-1), A[k].reshape(-1)
            assert bool((a[S == 0] == 0).all()), k
            worst = max(worst, float((a / (tw.C_BOUND * 2.0 ** -22 * S).clamp_min(1e-300)).max()))
        assert (worst < 1.0 / 64) == (power == 2.0), (power, worst)
