"""GPU tests of the per-atom PaiNN forward (csrc/painn.hip: k_painn_interaction_fwd<R>, the kernel of whole batches above
48 atoms and of the atom lists of oversized molecules) and of the LDS-staged vector form at F = 64
(k_painn_interaction_fwd_mol<R> on 256 threads): every element of q_out and mu_out against the fp64 twin with the
a-priori bound c_fwd_atom(R, D) u S, u = 2^-24 (tests/painn_tile_twin.py), on the 96-atom edge list of
test_gpu_painn_tile (in-degrees 0 .. 70: lists of more than one 16-edge chunk, of more than 64 edges) at R in
(8, 16, 20, 32) and F in (128, 64: 64-thread blocks); NaN-filled outputs, the proof that one dropped term is seen,
eight launches bit-identical."""
import numpy as np
import pytest
import torch

import painn_tile_twin as tw
from elementwise import assert_repeatable, assert_sees_a_dropped_term, assert_within, pick_term
from helpers import t
from test_gpu_painn_tile import N_ATOMS, _edges

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _ptr(x):
    return None if x is None else x.data_ptr()


def _random_inputs(N, E, F, R, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    return dict(q=rnd(N, F), mu=rnd(N, 3, F), xc=rnd(N, 3 * F), Wf=rnd(3 * F, R, scale=0.3), bf=rnd(3 * F, scale=0.2)), g


def _check(what, got, ref, cc, terms_of):
    for name, g in zip(("q_out", "mu_out"), got):
        r, S = ref[name]
        g = g.cpu()
        live = S > 0
        w = float(((g.double() - r).abs()[live] / (tw.U24 * S[live])).max())
        print("%s %s: worst error %.2f u S (bound %.2f, u = 2^-24)" % (what, name, w, cc))
        assert_within(g, r, S, cc, tw.U24, "%s %s" % (what, name))
        # one edge's term removed from the reference: flagged, and only its element
        terms, i = ref[terms_of[name]], ref["i"]
        bound = (cc * tw.U24 * S + (g.double() - r).abs())[i]
        k, ratio = pick_term(terms, bound, torch.ones_like(terms, dtype=torch.bool))
        assert ratio >= 2.0, (what, name, "no term stands above twice its bound", ratio)
        idx = tuple(int(v) for v in np.unravel_index(k, tuple(terms.shape)))
        assert_sees_a_dropped_term(g, r, S, cc, tw.U24, (int(i[idx[0]]),) + idx[1:], float(terms[idx]), "%s %s" % (what, name))


_TERMS = dict(q_out="terms_q", mu_out="terms_mu")


@pytest.mark.parametrize("F", [128, 64])
@pytest.mark.parametrize("R", [8, 16, 20, 32])
def test_per_atom_forward_every_element_against_the_twin(R, F):
    from geossl_amd import _lib
    from geossl_amd.layout import get_edge_layout
    ei, deg = _edges()
    E = ei.shape[1]
    c, g = _random_inputs(N_ATOMS, E, F, R, 500 + R + F)
    dirv = torch.randn(E, 3, generator=g)
    c.update(phi=torch.rand(E, R, generator=g).to(DEV), fcut=torch.rand(E, generator=g).to(DEV),
             dirv=(dirv / dirv.norm(dim=1, keepdim=True)).to(DEV))
    eit = t(ei, DEV)
    el = get_edge_layout(torch.zeros(N_ATOMS, dtype=torch.long, device=DEV), eit, 1)
    inc_ptr, inc_idx = el.inc["i"]
    assert np.array_equal(np.diff(inc_ptr.cpu().numpy()), np.asarray(deg)) and max(deg) == tw.MAX_DEGREE > 64

    def launch():
        q_out, mu_out = torch.full((N_ATOMS, F), NAN, device=DEV), torch.full((N_ATOMS, 3, F), NAN, device=DEV)
        _lib.call("geossl_painn_interaction_fwd", _ptr(c["q"]), _ptr(c["mu"]), _ptr(c["xc"]), _ptr(el.idx_j), _ptr(inc_ptr),
                  _ptr(inc_idx), _ptr(c["phi"]), _ptr(c["fcut"]), _ptr(c["dirv"]), _ptr(c["Wf"]), _ptr(c["bf"]), N_ATOMS, F, R,
                  _ptr(q_out), _ptr(mu_out), _lib.stream())
        torch.cuda.synchronize()
        return q_out, mu_out

    got = launch()
    ref = tw.forward(c["q"], c["mu"], c["xc"], el.idx_i, el.idx_j, c["phi"], c["fcut"], c["dirv"], c["Wf"], c["bf"])
    ref["i"] = el.idx_i.cpu().long()
    what = "per-atom fwd R=%d F=%d" % (R, F)
    _check(what, got, ref, tw.c_fwd_atom(R, tw.MAX_DEGREE), _TERMS)
    assert_repeatable(launch, got, what)


def test_staged_vector_forward_at_64_features_on_a_ragged_batch():
    """geossl_painn_interaction_fwd_mol at F = 64, R = 20: 256-thread blocks (four atoms of a molecule at a time), a dozen
    molecules of 1 to 33 atoms with real radius-graph geometry."""
    from geossl_amd import _lib
    from test_gpu_round3 import _painn_edge_case
    F, R, sizes = 64, 20, [2, 26, 1, 7, 18, 1, 12, 25, 3, 20, 9, 33]
    geo = _painn_edge_case(sizes, seed=5, R=R)                 # (its F = 128 tensors are not used)
    lay, el, N = geo["lay"], geo["el"], geo["N"]
    c, _ = _random_inputs(N, geo["E"], F, R, 77)
    c.update(phi=geo["phi"], fcut=geo["fcut"], dirv=geo["dirv"])
    inc_ptr, inc_idx = el.inc["i"]
    D = int((inc_ptr[1:] - inc_ptr[:-1]).max())
    assert lay.max_n == 33 and min(sizes) == 1 and D > 16       # more than one chunk of the edge stage

    def launch():
        q_out, mu_out = torch.full((N, F), NAN, device=DEV), torch.full((N, 3, F), NAN, device=DEV)
        _lib.call("geossl_painn_interaction_fwd_mol", _ptr(c["q"]), _ptr(c["mu"]), _ptr(c["xc"]), _ptr(el.idx_j), _ptr(inc_ptr),
                  _ptr(inc_idx), _ptr(c["phi"]), _ptr(c["fcut"]), _ptr(c["dirv"]), _ptr(c["Wf"]), _ptr(c["bf"]),
                  _ptr(lay.mol_ptr), lay.B, lay.max_n, N, F, R, _ptr(q_out), _ptr(mu_out), _lib.stream())
        torch.cuda.synchronize()
        return q_out, mu_out

    got = launch()
    ref = tw.forward(c["q"], c["mu"], c["xc"], el.idx_i, el.idx_j, c["phi"], c["fcut"], c["dirv"], c["Wf"], c["bf"])
    ref["i"] = el.idx_i.cpu().long()
    what = "fwd_mol F=64 R=20 D=%d" % D
    _check(what, got, ref, tw.c_fwd_atom(R, D), _TERMS)
    assert_repeatable(launch, got, what)
