"""GPU tests of the matrix-pipe PaiNN forward (csrc/painn_mma.hip: k_painn_fwd_mma<R, MZ>) through its C ABI
(geossl_painn_interaction_fwd_mma[_dyn]) with LIVE mu: every element of q_out and mu_out against the fp64 twin with the
a-priori bound c_fwd_mma(D) u S (tests/painn_tile_twin.py; outputs pre-filled with NaN, no element excluded: where S = 0
the result equals the reference exactly), launch-to-launch repeatability, and the proof that the checker sees a dropped
W_2 x_2 mu_j term on lanes 48-63 - the failure this kernel family once had.
  occupancy:  1024 molecules (two blocks per CU and two molecules per persistent block on set A; one block per CU on set B;
              a ragged batch), phi / fcut / dir from geossl_painn_edge_geom, the fp64 reference built on the device
  hand-made:  molecules of 44, 1, 2, 44 and 7 atoms with in-degrees 0 .. 43 (tests/painn_mma_case.py): runs of groups that
              cross and that end with a tile, molecules of 0 and 1 groups mod 8, mu given and NULL
  scales:     filter weights times 2^-30 and 2^20, zero weights, zero bias, both zero, fcut = 0 on a third of the edges,
              xc times 2^-20
  skip/list:  molecules above 44 atoms keep their NaN rows in the staged launch and are filled, exactly those rows, by
              geossl_painn_interaction_fwd_atoms over a shuffled list with dyn_nlist (bound c_fwd_atom(R, D) u24 S)
  refusals:   R = 12, R = 32 and F = 64 return hipErrorInvalidValue and write nothing."""
import numpy as np
import pytest
import torch

import packed_opsel_registry as reg
import painn_mma_case as hc
import painn_tile_twin as tw
from elementwise import assert_repeatable, assert_sees_a_dropped_term, assert_within, pick_term
from helpers import t
from objective_harness import lib_loaded  # noqa: F401 (the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
F = 128
INVALID = 1   # hipErrorInvalidValue


def _ptr(x):
    return None if x is None else x.data_ptr()


def _launch(c, mu="given", max_n=None, grp_end=None, R=None, Fv=F, outs=None):
    """One call of geossl_painn_interaction_fwd_mma_dyn (the exact entry point when max_n and grp_end are left alone) into
    NaN-filled outputs (or `outs`) -> (q_out, mu_out, rc)."""
    from geossl_amd import _lib
    lay, el = c["lay"], c["el"]
    row_edge, grp_atom, _, mol_grp = el.groups("i", lay.mol_ptr)
    mu_t = c["mu"] if isinstance(mu, str) else mu
    q_out, mu_out = outs if outs is not None else (torch.full((c["N"], F), NAN, device=DEV),
                                                   torch.full((c["N"], 3, F), NAN, device=DEV))
    head = (_ptr(c["q"]), _ptr(mu_t), _ptr(c["xc"]), _ptr(el.idx_j), _ptr(row_edge), _ptr(grp_atom), _ptr(mol_grp),
            _ptr(c["phi"]), _ptr(c["fcut"]), _ptr(c["dirv"]), _ptr(c["Wf"]), _ptr(c["bf"]), _ptr(lay.mol_ptr), lay.B,
            lay.max_n if max_n is None else max_n, c["N"], Fv, c["R"] if R is None else R, _ptr(q_out), _ptr(mu_out))
    lib = _lib.load()
    if max_n is None and grp_end is None:
        rc = lib.geossl_painn_interaction_fwd_mma(*head, _lib.stream())
    else:
        rc = lib.geossl_painn_interaction_fwd_mma_dyn(*head, _ptr(grp_end), _lib.stream())
    torch.cuda.synchronize()
    return q_out, mu_out, rc


def _twin(c, mu="given", device="cpu"):
    mu_t = c["mu"] if isinstance(mu, str) else mu
    return tw.forward(c["q"], mu_t, c["xc"], c["el"].idx_i, c["el"].idx_j, c["phi"], c["fcut"], c["dirv"], c["Wf"], c["bf"],
                      device=device)


def _max_in_degree(c):
    iptr = c["el"].inc["i"][0]
    return int((iptr[1:] - iptr[:-1]).max())


def _check(what, got, ref, cc, u=tw.U, rows=None):
    """Every element of (q_out, mu_out) - of the atoms `rows` when given - inside cc u S; prints the worst ratio."""
    worst = []
    for name, g in zip(("q_out", "mu_out"), got):
        r, S = ref[name]
        g = g.to(r.device)
        if rows is not None:
            g, r, S = g[rows], r[rows], S[rows]
        live = S > 0
        w = float(((g.double() - r).abs()[live] / (u * S[live])).max()) if bool(live.any()) else 0.0
        worst.append(w)
        print("%s %s: worst error %.2f u S (bound %.2f, u = 2^%d)" % (what, name, w, cc, round(np.log2(u))))
        assert_within(g, r, S, cc, u, "%s %s" % (what, name))
    return worst


def _sees_a_dropped_mu_term(what, c, got_mu, ref, cc):
    """One edge's W_2 x_2 mu_j[d] removed from the reference of mu_out, d in (y, z) and f % 32 >= 16 - lanes 48-63 of this
    kernel (lane = 32 kh + j, f = 32 m + j, and the half kh = 1 keeps y and z): flagged, and only that element."""
    r, S = ref["mu_out"]
    terms = ref["terms_mu_m"]
    i = c["el"].idx_i.to(r.device).long()
    got = got_mu.to(r.device)
    bound = (cc * tw.U * S + (got.double() - r).abs())[i]
    where = torch.zeros_like(terms, dtype=torch.bool)
    where[:, 1:, :] = (torch.arange(F, device=r.device) % 32 >= 16)[None, None, :]
    k, ratio = pick_term(terms, bound, where)
    assert ratio >= 2.0, (what, "no mu_j term stands above twice its bound", ratio)
    e, d, f = (int(v) for v in np.unravel_index(k, tuple(terms.shape)))
    assert d in (1, 2) and f % 32 >= 16
    assert_sees_a_dropped_term(got, r, S, cc, tw.U, (int(i[e]), d, f), float(terms[e, d, f]), what)


# ------------------------------------------------------------------------------------------------------- occupancy
_OCC = [("setA", 8), ("setA", 16), ("setA", 20), ("setB", 20), ("setB", 16), ("ragged", 20), ("ragged", 16)]


@pytest.mark.parametrize("sizes,R", _OCC, ids=["%s-R%d" % p for p in _OCC])
def test_forward_with_live_mu_at_full_occupancy_vs_fp64(sizes, R):
    """k_painn_fwd_mma<R, false> on 1024 molecules with mu drawn normal.  Set A: the smallest batch with two resident blocks
    per CU (two waves per SIMD, the regime of the round-6 failure) and two molecules per persistent block."""
    from geossl_amd.synthetic import molecule_sizes
    from test_gpu_packed_kernels import assert_occupancy
    from test_gpu_round3 import _painn_edge_case
    from test_gpu_round6 import _MU0_SIZES
    sz = _MU0_SIZES[sizes] if _MU0_SIZES[sizes] is not None else [int(n) for n in molecule_sizes(1024, "B")]
    assert len(sz) == reg.BENCH_MOLS
    c = _painn_edge_case(sz, seed=3, R=R)
    lay = c["lay"]
    lds = reg.painn_mma_lds(lay.max_n)
    grid = reg.painn_mma_grid(lay.B, lds)
    if sizes in ("setA", "setB"):
        assert lay.max_n <= (reg.SET_A_MAX_N if sizes == "setA" else reg.SET_B_MAX_N)
        waves = assert_occupancy(r"k_painn_fwd_mmaILi%dELb0E" % R, "R=%d set %s" % (R, sizes[-1]), lds=lds, grid=grid)
        assert waves == (2 if sizes == "setA" else 1)
    if sizes == "setA":
        assert grid == 2 * reg.CUS and lay.B == 2 * grid       # two blocks per CU, two molecules per block
    assert float(c["mu"].abs().mean()) > 0.5                    # mu is live (drawn normal)
    D = _max_in_degree(c)
    cc = tw.c_fwd_mma(D)
    q_out, mu_out, rc = _launch(c)
    assert rc == 0
    ref = _twin(c, device=DEV)
    what = "mma %s R=%d D=%d" % (sizes, R, D)
    _check(what, (q_out, mu_out), ref, cc)
    _sees_a_dropped_mu_term(what, c, mu_out, ref, cc)
    del ref
    assert_repeatable(lambda: _launch(c)[:2], (q_out, mu_out), what)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------- hand-made
_HAND = {}


def _hand_case(R):
    if R in _HAND:
        return _HAND[R]
    from geossl_amd.layout import MolLayout, get_edge_layout
    ei, batch = hc.edges()
    E, N = ei.shape[1], len(batch)
    g = torch.Generator().manual_seed(300 + R)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    dirv = torch.randn(E, 3, generator=g)
    dirv = (dirv / dirv.norm(dim=1, keepdim=True)).to(DEV)
    bt, eit = t(batch, DEV), t(ei, DEV)
    c = dict(R=R, E=E, N=N, q=rnd(N, F), mu=rnd(N, 3, F), xc=rnd(N, 3 * F), phi=torch.rand(E, R, generator=g).to(DEV),
             fcut=torch.rand(E, generator=g).to(DEV), dirv=dirv, Wf=rnd(3 * F, R, scale=0.3), bf=rnd(3 * F, scale=0.2),
             lay=MolLayout(bt, len(hc.SIZES), sizes=list(hc.SIZES)), ei=eit)
    c["el"] = get_edge_layout(bt, eit, len(hc.SIZES))
    _HAND[R] = c
    return c


def test_hand_made_layout_has_the_stated_groups():
    """From el.groups("i", mol_ptr) itself: the degrees, a run of groups across a tile's end, a run that ends with its tile,
    molecules of 0 and of 1 groups mod 8 - and the numpy restatement the CPU emulation walks is this layout."""
    c = _hand_case(20)
    row_edge, grp_atom, grp_ptr, mol_grp = (x.cpu().numpy() for x in c["el"].groups("i", c["lay"].mol_ptr))
    iptr = c["el"].inc["i"][0].cpu().numpy()
    deg = np.diff(iptr)
    assert set(hc.REQUIRED_DEGREES) <= set(deg[:44].tolist()) and deg.max() == hc.MAX_DEGREE == _max_in_degree(c)
    assert np.array_equal(c["lay"].mol_ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(hc.SIZES)]))
    per_mol = np.diff(mol_grp)
    assert 0 in (per_mol % 8).tolist() and 1 in (per_mol % 8).tolist()
    first, last = grp_ptr[:44] - mol_grp[0], grp_ptr[1:45] - 1 - mol_grp[0]
    assert any(f // 8 != l // 8 for f, l in zip(first, last))
    assert any(l % 8 == 7 and f // 8 == l // 8 for f, l in zip(first, last))
    re_np, code_np, gp_np, mg_np = hc.groups_np(c["ei"].cpu().numpy(), hc.SIZES)
    G = int(gp_np[-1])
    assert np.array_equal(grp_ptr, gp_np) and np.array_equal(mol_grp, mg_np)
    assert np.array_equal(row_edge[:4 * G], re_np) and np.array_equal(grp_atom[:G], code_np)
    assert bool((row_edge[4 * G:] == -1).all()) and bool((grp_atom[G:] == -1).all())


@pytest.mark.parametrize("R", [8, 16, 20])
def test_hand_made_molecules_every_element_against_the_twin(R):
    c = _hand_case(R)
    cc = tw.c_fwd_mma(hc.MAX_DEGREE)
    assert cc == 24.0
    got = _launch(c)
    assert got[2] == 0
    ref = _twin(c)
    what = "mma hand-made R=%d" % R
    _check(what, got[:2], ref, cc)
    _sees_a_dropped_mu_term(what, c, got[1], ref, cc)
    assert_repeatable(lambda: _launch(c)[:2], got[:2], what)
    # mu = NULL (k_painn_fwd_mma<R, true>): the twin with mu identically zero, and the bits of a run on a tensor of zeros
    zeros = torch.zeros_like(c["mu"])
    gn, gz = _launch(c, mu=None), _launch(c, mu=zeros)
    assert gn[2] == 0 and gz[2] == 0
    _check(what + " mu=NULL", gn[:2], _twin(c, mu=None), cc)
    assert torch.equal(gn[0], gz[0]) and torch.equal(gn[1], gz[1])
    assert_repeatable(lambda: _launch(c, mu=None)[:2], gn[:2], what + " mu=NULL")


_SCALES = ["wb_2m30", "wb_2p20", "b0", "w0", "both0", "fcut0", "xc_2m20"]


@pytest.mark.parametrize("kind", _SCALES)
def test_operand_scales_on_the_hand_made_molecules(kind):
    c = dict(_hand_case(20))
    if kind in ("wb_2m30", "wb_2p20"):
        s = 2.0 ** (-30 if kind == "wb_2m30" else 20)
        c["Wf"], c["bf"] = c["Wf"] * s, c["bf"] * s
    if kind in ("b0", "both0"):
        c["bf"] = torch.zeros_like(c["bf"])
    if kind in ("w0", "both0"):
        c["Wf"] = torch.zeros_like(c["Wf"])
    if kind == "fcut0":
        c["fcut"] = c["fcut"].clone()
        c["fcut"][::3] = 0.0
    if kind == "xc_2m20":
        c["xc"] = c["xc"] * 2.0 ** -20
    got = _launch(c)
    assert got[2] == 0
    _check("mma hand-made R=20 %s" % kind, got[:2], _twin(c), tw.c_fwd_mma(hc.MAX_DEGREE))
    if kind == "both0":   # a zero filter (the exponent floor of the weight scale): the identities, bit for bit
        assert torch.equal(got[0], c["q"]) and torch.equal(got[1], c["mu"])
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())


# ------------------------------------------------------------------------------------------------- skip and list forms
@pytest.mark.parametrize("R", [20, 8])
def test_staged_launch_skips_large_molecules_and_the_atom_list_fills_exactly_them(R):
    from geossl_amd import _lib
    from test_gpu_round3 import _painn_edge_case
    sizes = [18, 45, 7, 60, 44]
    c = _painn_edge_case(sizes, seed=3, R=R)
    lay, el, N = c["lay"], c["el"], c["N"]
    assert lay.max_n == 60
    big = torch.zeros(N, dtype=torch.bool, device=DEV)
    off = np.concatenate([[0], np.cumsum(sizes)])
    for m in (1, 3):
        big[off[m]:off[m + 1]] = True
    small = ~big
    D = _max_in_degree(c)
    ref = _twin(c)
    what = "mma skip R=%d D=%d" % (R, D)
    _, _, _, mol_grp = el.groups("i", lay.mol_ptr)
    q_out, mu_out, rc = _launch(c, max_n=60)
    assert rc == 0
    fill = torch.full((1,), NAN, device=DEV).view(torch.int32)
    for o in (q_out, mu_out):   # the rows of the 45- and 60-atom molecules keep their NaN bit patterns
        assert bool((o[big].view(torch.int32) == fill).all())
    _check(what + " staged rows", (q_out, mu_out), ref, tw.c_fwd_mma(D), rows=small.cpu())
    # mol_grp_end given explicitly: the bits of the NULL form
    q2, mu2, rc = _launch(c, max_n=60, grp_end=mol_grp[1:].contiguous())
    assert rc == 0
    for a, b in ((q2, q_out), (mu2, mu_out)):
        assert torch.equal(a[small], b[small]) and bool((a[big].view(torch.int32) == fill).all())
    # the atom list: lay.big_atoms(44), shuffled, in a buffer longer than the real count (the tail names atoms of the
    # staged molecules: a launch that read past dyn_nlist would rewrite their rows)
    lst, n_big, _ = lay.big_atoms(44)
    assert n_big == 105 and sorted(lst[:n_big].cpu().tolist()) == big.nonzero().flatten().cpu().tolist()
    perm = torch.from_numpy(np.random.default_rng(9).permutation(n_big)).to(DEV)
    buf = torch.cat([lst[:n_big][perm], torch.arange(0, 18, dtype=torch.int32, device=DEV)]).contiguous()
    dyn = torch.tensor([n_big], dtype=torch.int32, device=DEV)
    inc_ptr, inc_idx = el.inc["i"]
    before = (q_out.clone(), mu_out.clone())

    def fill_rows(outs):
        _lib.call("geossl_painn_interaction_fwd_atoms", _ptr(c["q"]), _ptr(c["mu"]), _ptr(c["xc"]), _ptr(el.idx_j),
                  _ptr(inc_ptr), _ptr(inc_idx), _ptr(c["phi"]), _ptr(c["fcut"]), _ptr(c["dirv"]), _ptr(c["Wf"]), _ptr(c["bf"]),
                  _ptr(buf), buf.numel(), _ptr(dyn), F, R, _ptr(outs[0]), _ptr(outs[1]), _lib.stream())
        torch.cuda.synchronize()
        return outs

    fill_rows((q_out, mu_out))
    for a, b in zip((q_out, mu_out), before):
        assert torch.equal(a[small], b[small])                 # no other row changes
    _check(what + " listed rows", (q_out, mu_out), ref, tw.c_fwd_atom(R, D), u=tw.U24, rows=big.cpu())
    assert_repeatable(lambda: fill_rows((before[0].clone(), before[1].clone())), (q_out, mu_out), what + " list")


# --------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("R,Fv", [(12, 128), (32, 128), (20, 64)])
def test_unserved_shapes_are_refused_and_write_nothing(R, Fv):
    c = _hand_case(20)
    fill = torch.full((1,), NAN, device=DEV).view(torch.int32)
    for kw in (dict(), dict(max_n=44)):                        # both entry points
        q_out, mu_out, rc = _launch(c, R=R, Fv=Fv, **kw)
        assert rc == INVALID
        assert bool((q_out.view(torch.int32) == fill).all()) and bool((mu_out.view(torch.int32) == fill).all())
