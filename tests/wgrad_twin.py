"""fp64 twin of the weight-gradient column GEMM (csrc/wgrad.h: k_wgrad_split<NCM, NCN, PlainOps, PIECES>; csrc/tn.h and
csrc/gemm.hip: geossl_tn_plan, k_reduce_multi; reached through ops.linear_wgrad and geossl_linear_wgrad[_dyn]) with
element-wise bounds, the catalogue of launch forms the code base issues and the operands the tests run them on.

A plain module (no tests).  `wgrad` returns per problem the fp64 values ref_dW = A[:R, :M]^T B[:R, :N] (+ prior) and
ref_db = column sums of A (+ prior), and S_dW / S_db, the same expressions on absolute values, so that a kernel is held
to |got - ref| <= c u S per element (tests/elementwise.py).

Operand model, per scale group of the kernel and not coarser.  PIECES = 2 (two fp16 pieces, u = 2^-22): a row chunk of
`chunk` rows (geossl_tn_plan) is taken in tiles of 32 rows; every 32-column operand block carries a RUNNING exponent
inside its chunk, e_t = max(e_{t-1}, mag_exponent(max |x| over the block's 32 x 32 elements of tile t)), and the tile's
elements are cut into h = fp16(x s), l = fp16(x s - h) under s = 2^(14 - e_t) (split.h: split2h_scaled, mag_exponent).
The running maximum m_t of the block over tiles 0..t of the chunk then sits in [2^13, 2^14) after scaling; h + l
carries 22 bits of x s while l is a normal fp16 number and an absolute error of at most 2^-25 (half of fp16's subnormal
spacing 2^-24) below that.  2^-25 against a maximum of at least 2^13 is 2^-38 = u 2^-16 of m_t:
        fl(x) = |x| + f max(m_t, 2^-101),      f = 2^-16                               (FLOOR_F)
(mag_exponent floors e at -100, so a block whose running maximum is below 2^-101 is scaled as if it were 2^-101).  A
spike in the last tile of a chunk raises the floor of that tile alone: earlier tiles were cut under their own, smaller
m_t, and the accumulator rescale that follows the exponent is a multiplication by a power of two (exact).  B is
modelled the same way.  PIECES = 3 (three bf16 pieces, no scales, u = 2^-24): fl(x) = |x|.  db is an fp32 sum of the
operand itself: S_db = sum |a|, u = 2^-24.  An accumulated prior adds |prior| to S.

`emulate` is the kernel's arithmetic on the CPU (numpy): the constants c of the bound are fixed from its error against
`ref` (tests/test_wgrad_twin_cpu.py), never from the kernel under test."""
import math

import numpy as np
import torch

from chain_twin import _f32, _split_bf16, _split_fp16, mag_exponent

FLOOR_F = 2.0 ** -16
U = {"two-piece": 2.0 ** -22, "bf16x3": 2.0 ** -24, "db": 2.0 ** -24}
# c of |got - ref| <= c u S: four times the worst err / (u S) of `emulate` against `ref` over the CPU grid, rounded up to
# a power of two (test_wgrad_twin_cpu.py: test_bound_constants_are_the_emulated_ones)
C_BOUND = {"two-piece": 16.0, "bf16x3": 16.0, "db": 16.0}
TN_MAX = 32
BLOCK_SCALES = (0, 7, -9, 3)
SPIKE = 2.0 ** 20
GUARD = 8


def family(pieces):
    return "two-piece" if pieces == 2 else "bf16x3"


def plan(R, nprob):
    """(chunk, nblk) of a launch: geossl_tn_plan, a host function of the library."""
    import ctypes as C
    from geossl_amd import _lib
    chunk, nblk = C.c_int(0), C.c_int(0)
    _lib.load().geossl_tn_plan(int(R), int(nprob), C.byref(chunk), C.byref(nblk))
    return chunk.value, nblk.value


# ----------------------------------------------------------------------------------------------------------- fp64 twin
def _fl(X, chunk, pieces, running=True):
    """fl of an operand [R, W] (fp64 magnitudes |x| in, model out).  `running=False` is the coarser model with one maximum
    per (chunk, block): what the bound must NOT be (the CPU test holds the two apart on `spike`)."""
    A = X.abs()
    if pieces == 3:
        return A
    R, W = A.shape
    Rp, Wp = -(-R // chunk) * chunk, -(-W // 32) * 32
    P = torch.zeros(Rp, Wp, dtype=torch.float64, device=A.device)
    P[:R, :W] = A
    mx = P.reshape(Rp // chunk, chunk // 32, 32, Wp // 32, 32).amax(dim=(2, 4))      # [chunks, tiles, blocks]
    mx = mx.cummax(dim=1)[0] if running else mx.amax(dim=1, keepdim=True).expand_as(mx)
    floor = FLOOR_F * mx.clamp_min(2.0 ** -101)
    floor = floor[:, :, None, :, None].expand(-1, -1, 32, -1, 32).reshape(Rp, Wp)
    return A + floor[:R, :W]


def wgrad(problems, R, M, N, chunk, prior=None, pieces=2, running=True):
    """problems: (A, B) or (A, B, ...) per problem, tensors with at least R rows and M / N columns.  prior: None or per
    problem (dW0 or None, db0 or None), the contents an accumulating launch adds to.  One dict per problem: ref_dW, S_dW
    [M, N], ref_db, S_db [M], and A, B (the fp64 operands, for the dropped-term proofs)."""
    out = []
    for z, pr in enumerate(problems):
        A, B = pr[0][:R, :M].double(), pr[1][:R, :N].double()
        ref, S = A.t() @ B, _fl(A, chunk, pieces, running).t() @ _fl(B, chunk, pieces, running)
        rb, Sb = A.sum(0), A.abs().sum(0)
        if prior is not None:
            w0, b0 = prior[z]
            if w0 is not None:
                ref, S = ref + w0[:M, :N].double(), S + w0[:M, :N].double().abs()
            if b0 is not None:
                rb, Sb = rb + b0[:M].double(), Sb + b0[:M].double().abs()
        out.append(dict(ref_dW=ref, S_dW=S, ref_db=rb, S_db=Sb, A=A, B=B))
    return out


def proof_rows(R, chunk):
    """Rows whose product term the dropped-term proofs remove: in the first tile of a chunk, in the last (partial) tile
    of the launch, in a tile served by the second request set (tile 1 of a chunk) and in a tile served after a refill
    (tile 2 or 3 of a chunk: chunk >= 128), where the launch has them: {name: row}."""
    last = (R - 1) // chunk * chunk                       # first row of the last chunk
    rows = {"first tile": min(last + 7, R - 1), "last tile": R - 1}
    base = (R // chunk - 1) * chunk if R >= chunk else 0  # the last full chunk (or the only, partial one)
    n = min(chunk, R - base)
    for name, tile, off in (("second set", 1, 11), ("after refill", 2, 13), ("second set after refill", 3, 5)):
        if n > 32 * tile:
            rows[name] = base + min(32 * tile + off, n - 1)
    return rows


def pick_dropped_term(d, r, c, u):
    """The product a[r][m] b[r][n] of row r that is largest against the bound of its element: ((m, n), term, ratio)."""
    from elementwise import pick_term
    terms = d["A"][r][:, None] * d["B"][r][None, :]
    pos, ratio = pick_term(terms, c * u * d["S_dW"], torch.ones_like(terms, dtype=torch.bool))
    idx = (pos // terms.size(1), pos % terms.size(1))
    return idx, terms[idx], ratio


# ---------------------------------------------------------------------------------------------------- arithmetic model
def _kahan32(parts):
    """kahan_sum_strided (common.h) over the leading axis, in fp32."""
    s = np.zeros(parts.shape[1:], np.float32)
    c = np.zeros_like(s)
    for p in parts:
        y = _f32(p - c)
        t = _f32(s + y)
        c = _f32(_f32(t - s) - y)
        s = t
    return s


def _reduce32(parts, prior):
    """reduce_multi_block (tn.h): four slices of the partial list, per = ceil(nblk / 4), each a compensated sum; then
    (prior or 0) + slice 0 + 1 + 2 + 3 in fp32, in that order."""
    nblk = parts.shape[0]
    per = (nblk + 3) // 4
    v = np.zeros(parts.shape[1:], np.float32) if prior is None else _f32(prior).copy()
    for s in range(4):
        v = _f32(v + _kahan32(parts[min(nblk, s * per):min(nblk, s * per + per)]))
    return v


def _chunk_partial(a, b, pieces):
    """One block of k_wgrad_split on its rows a [n, Mp], b [n, Np] (fp32, columns padded with zeros to blocks of 32,
    n <= chunk): the dW partial [Mp, Np] and the db partial [Mp]."""
    n, Mp = a.shape
    Np = b.shape[1]
    nbm, nbn = Mp // 32, Np // 32
    acc = np.zeros((Mp, Np), np.float32)
    ea, eb = np.full(nbm, -100, np.int64), np.full(nbn, -100, np.int64)
    eacc = np.full((nbm, nbn), -200, np.int64)
    bsum = np.zeros((2, Mp), np.float32)      # per half-wave kh: the lane's sequential sum
    for row0 in range(0, n, 32):
        ta, tb = np.zeros((32, Mp), np.float32), np.zeros((32, Np), np.float32)
        k = min(32, n - row0)
        ta[:k], tb[:k] = a[row0:row0 + k], b[row0:row0 + k]      # (rows past row_end are zero: finish_col8)
        for ks in range(2):
            for q in range(8):
                for kh in range(2):
                    bsum[kh] = _f32(bsum[kh] + ta[16 * ks + 8 * kh + q])
        if pieces == 3:
            pa, pb = _split_bf16(ta), _split_bf16(tb)
            order = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))         # mma6: l h, h l, m m, m h, h m, h h
        else:
            ea = np.maximum(ea, mag_exponent(np.abs(ta).reshape(32, nbm, 32).max(axis=(0, 2))))
            eb = np.maximum(eb, mag_exponent(np.abs(tb).reshape(32, nbn, 32).max(axis=(0, 2))))
            pa = _split_fp16(ta.astype(np.float64) * np.exp2((14 - np.repeat(ea, 32)).astype(np.float64))[None, :])
            pb = _split_fp16(tb.astype(np.float64) * np.exp2((14 - np.repeat(eb, 32)).astype(np.float64))[None, :])
            order = ((1, 0), (0, 1), (0, 0))                                   # l h, h l, h h
            en = ea[:, None] + eb[None, :]
            f = np.exp2((eacc - en).astype(np.float64)).astype(np.float32)     # (ldexpf: 0 when it underflows)
            acc = _f32(acc * np.repeat(np.repeat(f, 32, axis=0), 32, axis=1))
            eacc = en
        for ks in range(2):
            rows = slice(16 * ks, 16 * ks + 16)
            for i, j in order:   # one MFMA: the exact sum of its 16 products added with one rounding
                acc = _f32(acc.astype(np.float64) + pa[i][rows].astype(np.float64).T @ pb[j][rows].astype(np.float64))
    if pieces == 2:
        kk = np.exp2((eacc - 28).astype(np.float64)).astype(np.float32)
        acc = _f32(acc * np.repeat(np.repeat(kk, 32, axis=0), 32, axis=1))
    return acc, _f32(bsum[0] + bsum[1])


def emulate(problems, R, M, N, chunk, prior=None, pieces=2):
    """The kernels' arithmetic on the CPU, per problem (dW [M, N], db [M]) as float32 arrays: per row chunk the running
    block exponents and scales 2^(14 - e), the two fp16 pieces (or three bf16 pieces, unscaled), the piece products
    summed in fp32 per 32-row tile in two 16-wide k-steps, the accumulator rescale, the final 2^(eacc - 28), the per-lane
    sequential bias sums and their pair sum; then the four-slice compensated reduction in slice order and the
    `accumulate` add.  A model for fixing c: it need not give the GPU's bits."""
    Mp, Np = -(-M // 32) * 32, -(-N // 32) * 32
    out = []
    for z, pr in enumerate(problems):
        a, b = np.zeros((R, Mp), np.float32), np.zeros((R, Np), np.float32)
        a[:, :M] = pr[0][:R, :M].detach().cpu().numpy()           # (columns past M / N are zeroed by the kernel)
        b[:, :N] = pr[1][:R, :N].detach().cpu().numpy()
        parts = [_chunk_partial(a[r0:r0 + chunk], b[r0:r0 + chunk], pieces) for r0 in range(0, R, chunk)]
        w0 = b0 = None
        if prior is not None:
            w0, b0 = prior[z]
            w0 = None if w0 is None else w0[:M, :N].detach().cpu().numpy()
            b0 = None if b0 is None else b0[:M].detach().cpu().numpy()
        dW = _reduce32(np.stack([p[0][:M, :N] for p in parts]), w0)
        db = _reduce32(np.stack([p[1][:M] for p in parts]), b0)
        out.append((dW, db))
    return out


# ------------------------------------------------------------------------------------------------- catalogue of forms
def nprob_class(n):
    return "one" if n == 1 else ("few" if n <= 8 else "many")


def db_class(dbs):
    given = [d is not None for d in dbs]
    return "all" if all(given) else ("mixed" if any(given) else "none")


def _form(M, N, wide, nprob, accumulate, db, dyn):
    return dict(M=M, N=N, wide=wide, nprob=nprob, accumulate=accumulate, db=db, dyn=dyn)


# Every launch form the code base issues: M, N; wide (a row stride above the width: column slices of wider tensors);
# the problem count (classes one / 2..8 / 9..32); accumulate; db given for all / none / some of the problems; the row
# count by value or as device data (_dyn).  (M, N, wide, nprob, accumulate, db, dyn), by the code that issues them:
_LAUNCHED = {
    # SchNet.backward (Geom3D/models/schnet.py: every atom-row gradient of the step in one launch; lin1 has no bias;
    # 18 problems at six interactions, 20 with the head's; a capacity bucket passes the row count as device data)
    "schnet": [(128, 128, False, 20, False, "mixed", False), (128, 128, False, 18, True, "mixed", False),
               (128, 128, False, 18, False, "mixed", True), (128, 128, False, 18, True, "mixed", True),
               (64, 64, False, 18, False, "mixed", False), (32, 32, False, 18, False, "mixed", False)],
    # PaiNN.backward (Geom3D/models/painn.py: groups keyed by (rows, lda, ldb, ldw), atom rows and 3 x atom rows)
    "painn": [(128, 128, False, 3, False, "all", False), (128, 128, False, 3, True, "all", False),
              (128, 128, False, 3, True, "all", True), (128, 128, False, 3, True, "none", False),
              (128, 128, True, 3, False, "mixed", False), (128, 128, True, 3, True, "mixed", False),
              (128, 128, True, 3, True, "mixed", True), (128, 128, True, 6, True, "none", False),
              (128, 128, True, 6, True, "none", True), (128, 128, True, 12, False, "all", False),
              (128, 128, True, 12, True, "all", False), (128, 128, True, 12, True, "all", True),
              (128, 128, True, 12, True, "none", False), (128, 128, False, 12, True, "none", False),
              (64, 64, True, 3, False, "mixed", False)],
    # the tape's second-order products (tape.py: _mm_launch "tn", one 128 x 128 tile per launch; the batched rounds of
    # weight gradients, accumulating from the second round on)
    "tape": [(32, 64, False, 1, False, "none", False), (64, 128, False, 1, False, "none", False),
             (128, 128, True, 1, False, "none", False), (128, 128, False, 1, False, "none", False),
             (32, 32, False, 1, False, "none", False),
             (128, 32, True, 12, False, "all", False), (128, 32, True, 12, True, "none", False),
             (128, 64, False, 3, False, "all", False), (128, 64, False, 3, True, "none", False),
             (128, 128, False, 12, False, "mixed", False), (128, 128, False, 12, True, "mixed", False)],
    # the 3D InfoGraph discriminator (ops._infograph_wgrad: F <= 128, and F = 256 as four 128-blocks of one launch)
    "infograph": [(128, 128, False, 1, False, "none", False), (128, 128, False, 1, True, "none", False),
                  (64, 64, False, 1, False, "none", False),
                  (128, 128, True, 4, False, "none", False), (128, 128, True, 4, True, "none", False)],
    # the property head's dW1 (ops._property_w1_grad: F <= 128, and F = 256 as two 128-column problems, db for the first)
    "property": [(64, 128, False, 1, False, "all", False), (64, 128, False, 1, True, "all", False),
                 (32, 64, False, 1, False, "all", False),
                 (128, 128, True, 2, False, "mixed", False), (128, 128, True, 2, True, "mixed", False)],
}


def _name(src, M, N, wide, nprob, accumulate, db, dyn):
    return "%s-%dx%d-%s-%d-%s%s%s" % (src, M, N, "wide" if wide else "tight", nprob, db, "-acc" if accumulate else "",
                                     "-dyn" if dyn else "")


FORMS = {}
_sigs = set()
for _src, _rows in _LAUNCHED.items():
    for _r in _rows:
        _sig = (_r[0], _r[1], _r[2], nprob_class(_r[3]), _r[4], _r[5], _r[6])
        if _sig not in _sigs:         # (two sources that launch the same form share its entry)
            _sigs.add(_sig)
            FORMS[_name(_src, *_r)] = _form(*_r)
KINDS = ("main", "blocks", "rising", "falling", "spike", "zeros", "slices", "shared")


def signature(M, N, wide, nprob, accumulate, db, dyn):
    """What the completeness check compares."""
    return (M, N, bool(wide), nprob_class(nprob), bool(accumulate), db, bool(dyn))


def form_signature(f):
    return signature(f["M"], f["N"], f["wide"], f["nprob"], f["accumulate"], f["db"], f["dyn"])


def db_given(form_db, nprob):
    """Which problems of a launch get a db: all, none, or (`mixed`) every problem but each third one, first one given."""
    return [form_db == "all" or (form_db == "mixed" and z % 3 != 1) for z in range(nprob)]


def operands(kind, nprob, R, M, N, chunk, seed=0):
    """[(A [R, M], B [R, N])] * nprob of fp32 CPU tensors from a seeded CPU generator (`slices` has the data of `main`:
    the test places it; `shared`: three problems on one A, whatever nprob says)."""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * R + 31 * M + N + 7 * nprob + len(kind))
    rn = lambda *shape: torch.randn(*shape, generator=g)
    if kind == "shared":
        A = rn(R, M)
        return [(A, rn(R, N)) for _ in range(3)]
    rows = torch.arange(R)
    tile_in_chunk = (rows % chunk) // 32
    nbm, nbn = -(-M // 32), -(-N // 32)
    cm, cn = torch.arange(M) // 32, torch.arange(N) // 32
    out = []
    for z in range(nprob):
        A, B = rn(R, M), rn(R, N)
        if kind == "blocks":
            sa = torch.tensor([BLOCK_SCALES[(b + z) % 4] for b in range(nbm)], dtype=torch.float32)
            sb = torch.tensor([BLOCK_SCALES[(b + 2 * z + 1) % 4] for b in range(nbn)], dtype=torch.float32)
            A, B = A * torch.exp2(sa)[cm][None, :], B * torch.exp2(sb)[cn][None, :]
        elif kind in ("rising", "falling"):
            sc = torch.exp2((3.0 if kind == "rising" else -3.0) * tile_in_chunk.float())[:, None]
            A, B = A * sc, B * sc
        elif kind == "spike":
            r = min(chunk, R) - 1           # the last row of the first chunk
            A[r, min(5, M - 1)] = SPIKE
            B[r, max(N - 3, 0)] = -SPIKE
        elif kind == "zeros":
            c = rows // chunk
            A[(c % 4 == 1)] = 0.0                                         # an all-zero chunk of A
            lead = (c % 4 != 1) & (c % 4 != 3) & (tile_in_chunk == 0)
            A[lead] = 0.0                                                 # all-zero leading tile: exponents at the floor
            tiny = (c % 4 == 0) & (tile_in_chunk == 1)
            A[tiny] = A[tiny] * 1e-30                                     # ... followed by 1e-30, then ordinary values
            B[(c % 4 == 2) & (tile_in_chunk == 0)] = 0.0
            if nbm > 1:
                A[:, 32:64] = 0.0                                         # an all-zero A block
            if z % 3 == 1 and nbn > 1:
                B[:, 32 * (nbn - 1):] = 0.0                               # an all-zero B block
            if z % 3 == 2:
                B.zero_()                                                 # an all-zero B
        out.append((A, B))
    return out


def priors(problems, M, N, given, seed=0):
    """Prefilled outputs of an accumulating launch: entries up to 2^10 times the size of the product's."""
    g = torch.Generator().manual_seed(77 + seed)
    out = []
    for z, (A, B) in enumerate(problems):
        R = A.size(0)
        sw = math.sqrt(R) * float(A.abs().max().clamp_min(1e-30)) * float(B.abs().max().clamp_min(1e-30)) / 9.0
        mag = torch.exp2(torch.randint(-4, 11, (M, N), generator=g).float())
        w0 = torch.randn(M, N, generator=g) * mag * sw
        b0 = torch.randn(M, generator=g) * mag[:, 0] * math.sqrt(R) * float(A.abs().max()) / 3.0
        out.append((w0, b0 if given[z] else None))
    return out
