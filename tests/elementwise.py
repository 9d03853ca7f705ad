"""Element-wise comparison with an a-priori bound, shared by the GPU tests that check kernels against fp64:
|got - ref| <= c u S (+ extra) per element, the proof that the checker sees one missing term, launch-to-launch
repeatability."""
import pytest
import torch

REPEATS = 8


def flagged(got, ref, S, c, u, extra=None):
    """Elements outside |got - ref| <= c u S (+ extra): a boolean tensor of got's shape (NaN and inf are outside)."""
    bound = c * u * S
    if extra is not None:
        bound = bound + extra
    err = (got.double() - ref).abs()
    return ~(err <= bound)


def assert_within(got, ref, S, c, u, what, extra=None):
    bad = flagged(got, ref, S, c, u, extra)
    n = int(bad.sum())
    if n:
        idx = bad.nonzero()[:8]
        rows = [(tuple(int(v) for v in i), float(got[tuple(i)]), float(ref[tuple(i)]), float(S[tuple(i)])) for i in idx]
        cs = "c" if torch.is_tensor(c) and c.numel() > 1 else "%g" % float(c)          # (c may differ by row)
        pytest.fail("%s: %d of %d elements outside %s u S (index, got, ref, S): %s" % (what, n, bad.numel(), cs, rows))


def assert_sees_a_dropped_term(got, ref, S, c, u, index, term, what, extra=None):
    """Remove `term` from ref[index]: the checker must flag exactly that element."""
    ref2 = ref.clone()
    ref2[index] -= term
    bad = flagged(got, ref2, S, c, u, extra)
    hit = [tuple(int(v) for v in i) for i in bad.nonzero()[:4]]
    assert hit == [tuple(int(v) for v in index)] and int(bad.sum()) == 1, (what, index, float(term), hit)


def pick_term(terms, bound, where):
    """Among the candidate terms (`where` True), the one largest against the bound of its element: (flat position,
    ratio).  A term under twice its bound cannot be told apart from rounding: the test then fails."""
    ratio = torch.where(where & (bound > 0), terms.abs() / bound, torch.zeros_like(terms))
    k = int(ratio.argmax())
    return k, float(ratio.reshape(-1)[k])


def assert_repeatable(launch, first, what):
    """Seven more launches, each compared with the first element by element."""
    for rep in range(REPEATS - 1):
        again = launch()
        for a, b in zip(first, again):
            n = int((a != b).sum()) + int((a.isnan() != b.isnan()).sum())
            assert n == 0, (what, rep, "%d elements differ between launches" % n)
