"""csrc/fused_ops.hip against float64 references, every op at its edges (MI355X only).

LayerNorm forward / backward (with and without the fused residual), bias + GELU, the column sums
(``col_reduce`` behind LayerNorm's dgamma / dbeta, the GELU and linear bias gradients, and the
batched ``col_reduce_multi`` / ``column_sum_parts_multi``) and the softmax cross-entropy are held,
element by element and output by output, to

    |got - ref| <= K_op 2^-24 M + FLOOR (+ extra)

``ref`` is the float64 reference of tests/fused_cases.py (anchored to float64 torch by
tests/test_fused_reference.py), M the magnitude of the terms summed into the element (written down
next to each reference), FLOOR = 2^-126 the float32 normal limit, ``extra`` the proven 1.5e-7 of the
A&S 7.1.26 erf polynomial (GELU only); a bf16 output adds one RNE rounding, E + 2^-8 (|ref| + E).
Every K_op is 2 x the largest ratio a float32 CPU emulation of the kernel's rounding points shows
against the same reference (fused_cases.py, held by test_fused_reference.py) -- emulated, not
fitted, never measured against a kernel.  The backward passes are referenced from the statistics
(mean, rstd, lse) they are *given*, so a forward error is not counted twice.

``split_sum_bf16``, ``embed_tokens_*``, ``patchify_u8`` and ``multi_copy`` have fully determined
arithmetic and are compared bitwise with the same operations in IEEE float32 torch.

The shapes are the smallest that reach each path of the launch geometry (fused_cases.py names the
path next to each): the K = 1 / 2 / 4 register layouts at C = 512 / 1024, the grid strides of
ln_fwd (> 16384 rows), ln_bwd (> 16384 rows, odd N: the clamped duplicate of the last row),
bias_gelu_fwd's second chunk and second sweep, xent_bwd / split_sum / multi_copy above 524288 work
items, col_reduce's rounds at R = 128, and the job-table limits 40 / 64.

Cross-entropy semantics (fixed with this file): a NaN logit or a row of only -inf gives a NaN lse
and loss on that row alone, -inf logits count as probability 0, a label outside [0, K) gives a NaN
row loss, a NaN mean loss and a NaN dz row (as csrc/head.hip).  Before the fix xent_fwd_kernel lost
a NaN logit that was alone in its lane (K <= 64), turned a row NaN when a lane's first logit was -inf,
and gave loss 0 with a non-zero gradient for an out-of-range label.

K_op, the emulated ratio it comes from, and the largest ratio measured on the MI355X over this file
(err / (2^-24 M) on fp32 outputs; no kernel needed more than its K):

    output            K    emulated   MI355X
    LN mean           7      3.02      3.02
    LN rstd           9      4.29      4.29
    LN y              5      2.08      2.10
    LN dx             6      2.56      2.80
    LN dgamma         4      1.85      1.51
    LN dbeta          7      3.08      2.27
    GELU y            5      2.05      2.37
    GELU dx           7      3.42      3.39
    GELU dbias        4      1.85      1.62
    column sums       5      2.49      2.82 (col_reduce alone), 1.33 (column_sum)
    xent lse          2      0.90      1.90
    xent row loss     3      1.32      1.47
    xent dz           4      1.51      1.76

The lse is the tightest: __expf / __logf are less exact than the correctly rounded functions of the
emulation, and 1.90 against K = 2 is what the factor 2 is there for.

With the cross-entropy fix reverted (scratch build) 22 of the 137 tests here fail: nan_logit at K = 10
(2; the K = 129 cases pass either way, a lane with a later finite logit keeps its NaN), the masked
K = 1000 lane_first case (2), only-the-label-finite at K = 65 and 129 (4), the row of only -inf (2), and
all 12 out-of-range-label cases.

Arithmetic-only mutations of csrc/fused_ops.hip (none moves an address; never committed), number of
the 137 tests here that fail:

    1. the variance divides by C - 1                                   30
    2. ``- m1`` dropped in ln_bwd                                      30
    3. ``&& live`` removed, the clamped row accumulates                31
    4. col_reduce's row stride kCrPh * 4                               29
    5. bias_gelu_fwd stores v[0] for the second chunk                   4
    6. gelu_grad's 0.39894... becomes 0.4                              16
    7. inv_n dropped in xent_bwd                                       38
    8. ln_fwd's K dispatch with ``C < 512``                             0
    8b. ln_fwd's K dispatch with ``C <= 520`` for K = 1                 8

Mutation 8 is an equivalent mutant, not a gap: at C = 512 the K = 2 layout masks its whole second
chunk (columns >= C) and the first chunk is the K = 1 layout, so every output keeps its bits; only the
register count changes.  8b moves the same boundary the harmful way (columns 512 .. 519 fall out of
the row) and is caught at C = 520.

Not covered: the R > 1 instantiations of ln_fwd_kernel (unreachable: ``multi`` is a constant false).
"""

from __future__ import annotations

import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fused_cases as fc  # noqa: E402
from p2pfl_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
WORST: dict = {}  # op -> largest err / (2^-24 M) seen on an fp32 output


@pytest.fixture(autouse=True)
def _require_ext():
    ops.ext()  # fail loudly if the native extension is missing on a GPU box


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print(f"largest GPU ratio {k}: {WORST[k]:.2f} x 2^-24 M")


def fx():
    return ops.ext().fused


def _dev(x, dtype=torch.float32):
    return x.to(DEV).to(dtype).contiguous()


def _bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _same_bits(label, got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, label
    n = int((_bits(got) != _bits(want)).sum())
    assert n == 0, f"{label}: {n} elements differ bitwise"


def _hold(label, got, ref, M, K, extra=None, where=None, op=None):
    """|got - ref| <= K 2^-24 M + FLOOR (+ extra), widened by one bf16 rounding for a bf16 ``got``, on the
    elements selected by ``where`` (default all), whose reference must be finite."""
    ref, M = ref.double(), M.double().expand_as(ref)
    sel = torch.ones_like(ref, dtype=torch.bool) if where is None else where.expand_as(ref)
    assert bool(torch.isfinite(ref[sel]).all()), f"{label}: the reference is not finite"
    E = fc.bound(K, M, None if extra is None else extra.double().expand_as(ref))
    if got.dtype == torch.bfloat16:
        E = fc.widen_bf16(E, ref)
    err = (got.double() - ref).abs()
    r = torch.where(sel, err / E, torch.zeros_like(err))
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    worst = float(r.max()) if r.numel() else 0.0
    if got.dtype == torch.float32 and op is not None and r.numel():
        raw = fc.ratio(got[sel], ref[sel], M[sel], None if extra is None else extra.double().expand_as(ref)[sel])
        WORST[op] = max(WORST.get(op, 0.0), raw)
    if worst > 1.0:
        i = int(r.argmax())
        pytest.fail(f"{label}: element {i}: got {float(got.reshape(-1)[i])!r} ref {float(ref.reshape(-1)[i])!r} "
                    f"err {float(err.reshape(-1)[i]):.3e} bound {float(E.reshape(-1)[i]):.3e} "
                    f"({worst * K:.2f} x 2^-24 M against K = {K}); {int((r > 1).sum())} elements outside", pytrace=False)
    return worst


# ----------------------------------------------------------------------------
# LayerNorm
# ----------------------------------------------------------------------------
def _ln_case(N, C, fam, eps, dtype, res, seed=0):
    bf = dtype == torch.bfloat16
    x = _dev(fc.act(fc.ln_values(fam, N, C, seed), bf), dtype)
    r = None
    if res:
        r = x.clone() if fam == "constant_rows" else _dev(fc.standard((N, C), "res", N, C), dtype)
    w, b = (_dev(t) for t in fc.ln_params(C))
    dy = _dev(fc.standard((N, C), "dy", N, C), dtype)
    gs = _dev(fc.standard((N, C), "gs", N, C), dtype) if res else None
    return x, r, w, b, dy, gs


def _ln_check(label, N, C, fam, eps, dtype, res):
    bf = dtype == torch.bfloat16
    x, r, w, b, dy, gs = _ln_case(N, C, fam, eps, dtype, res)
    out = fx().ln_fwd(x, w, b, eps, r)
    y, mean, rstd = out[:3]
    ref = fc.ln_fwd_ref(x, w, b, eps, r, bf)
    s = x
    if res:
        s = out[3]
        _same_bits(f"{label} sum", s, ref["s"].to(dtype))
    _hold(f"{label} mean", mean, ref["mean"], ref["Mmean"], fc.K_LN_MEAN, op="ln_mean")
    _hold(f"{label} rstd", rstd, ref["rstd"], ref["Mrstd"], fc.K_LN_RSTD, op="ln_rstd")
    _hold(f"{label} y", y, ref["y"], ref["My"], fc.K_LN_Y, op="ln_y")
    if fam == "constant_rows":  # variance exactly 0: d == 0, y == beta whatever rstd is
        _same_bits(f"{label} y == beta", y, b.expand(N, C).to(dtype).contiguous())
        _same_bits(f"{label} mean", mean, s[:, 0].float().contiguous())
    dx, dw, db = fx().ln_bwd(dy, s, w, mean, rstd, gs)
    bw = fc.ln_bwd_ref(dy, s, w, mean, rstd, gs)
    _hold(f"{label} dx", dx, bw["dx"], bw["Mdx"], fc.K_LN_DX, op="ln_dx")
    _hold(f"{label} dgamma", dw, bw["dw"], bw["Mdw"], fc.K_LN_DW, op="ln_dw")
    _hold(f"{label} dbeta", db, bw["db"], bw["Mdb"], fc.K_LN_DB, op="ln_db")
    return (y, mean, rstd, s, dx, dw, db), (x, r, w, b, dy, gs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", fc.LN_CS)
def test_layer_norm(C, dtype):
    for N in fc.LN_NS:
        for fam in fc.LN_FAMILIES:
            for eps in fc.LN_EPS:
                for res in (False, True):
                    _ln_check(f"ln N={N} C={C} {fam} eps={eps} res={res}", N, C, fam, eps, dtype, res)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,C", [fc.LN_FWD_STRIDE, fc.LN_BWD_STRIDE])
def test_layer_norm_grid_stride(N, C, dtype):
    for res in (False, True):
        _ln_check(f"ln N={N} C={C} res={res}", N, C, "standard", 1e-5, dtype, res)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [8, 520, 2048])
def test_layer_norm_through_ops(C, dtype):
    """ops.layer_norm / ops.add_layer_norm and their autograd give the bindings' bits."""
    N, eps = 5, 1e-5
    for res in (False, True):
        (y, mean, rstd, s, dx, dw, db), (x, r, w, b, dy, gs) = _ln_check(f"ln ops C={C}", N, C, "standard", eps, dtype, res)
        xa, wa, ba = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        if res:
            ra = r.clone().requires_grad_(True)
            s2, y2 = ops.add_layer_norm(xa, ra, wa, ba, eps)
            torch.autograd.backward([s2, y2], [gs, dy])
            _same_bits("add_layer_norm s", s2.detach(), s)
            _same_bits("add_layer_norm dr", ra.grad, dx)
        else:
            y2 = ops.layer_norm(xa, wa, ba, eps)
            y2.backward(dy)
        _same_bits("y", y2.detach(), y)
        _same_bits("dx", xa.grad, dx)
        _same_bits("dgamma", wa.grad, dw)
        _same_bits("dbeta", ba.grad, db)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("val", [math.nan, math.inf])
def test_layer_norm_poison_is_contained(val, dtype):
    """One NaN / Inf in x: only that row's y, mean, rstd and dx are non-finite (dgamma loses every column, as
    its reference does: xhat of the whole row is NaN).  One in dy: that row's dx, and dgamma / dbeta in that
    column only.  The last row is poisoned too in a second pass: its clamped duplicate (odd N) adds nothing."""
    N, C, eps = 5, 520, 1e-5
    for row, col in ((2, 517), (4, 0)):
        x, _, w, b, dy, _ = _ln_case(N, C, "standard", eps, dtype, False)
        x[row, col] = val
        rows = torch.arange(N, device=DEV).view(-1, 1) != row
        y, mean, rstd = fx().ln_fwd(x, w, b, eps)
        ref = fc.ln_fwd_ref(x, w, b, eps)
        assert not bool(torch.isfinite(y[row].float()).any()) and not bool(torch.isfinite(rstd[row]))
        assert bool(torch.isnan(mean[row])) == math.isnan(val) and (math.isnan(val) or float(mean[row]) == math.inf)
        _hold("poison y", y, ref["y"], ref["My"], fc.K_LN_Y, where=rows)
        _hold("poison mean", mean, ref["mean"], ref["Mmean"], fc.K_LN_MEAN, where=rows[:, 0])
        _hold("poison rstd", rstd, ref["rstd"], ref["Mrstd"], fc.K_LN_RSTD, where=rows[:, 0])
        dx, dw, db = fx().ln_bwd(dy, x, w, mean, rstd)
        bw = fc.ln_bwd_ref(dy, x, w, mean, rstd)
        assert not bool(torch.isfinite(dx[row].float()).any())
        _hold("poison dx", dx, bw["dx"], bw["Mdx"], fc.K_LN_DX, where=rows)
        assert not bool(torch.isfinite(bw["dw"]).any()) and not bool(torch.isfinite(dw).any())
        _hold("poison dbeta", db, bw["db"], bw["Mdb"], fc.K_LN_DB)
        # dy poisoned instead
        x, _, w, b, dy, _ = _ln_case(N, C, "standard", eps, dtype, False)
        dy[row, col] = val
        y, mean, rstd = fx().ln_fwd(x, w, b, eps)
        dx, dw, db = fx().ln_bwd(dy, x, w, mean, rstd)
        bw = fc.ln_bwd_ref(dy, x, w, mean, rstd)
        cols = torch.arange(C, device=DEV) != col
        assert not bool(torch.isfinite(dx[row].float()).any())
        assert not bool(torch.isfinite(dw[col])) and not bool(torch.isfinite(db[col]))
        _hold("poison dx", dx, bw["dx"], bw["Mdx"], fc.K_LN_DX, where=rows)
        _hold("poison dgamma", dw, bw["dw"], bw["Mdw"], fc.K_LN_DW, where=cols)
        _hold("poison dbeta", db, bw["db"], bw["Mdb"], fc.K_LN_DB, where=cols)


# ----------------------------------------------------------------------------
# column reductions
# ----------------------------------------------------------------------------
def _reduce_single(part, bf16_out=False):
    out = torch.empty(part.shape[1], device=DEV, dtype=torch.bfloat16 if bf16_out else torch.float32)
    fx().col_reduce_multi([part], [out])
    return out


@pytest.mark.parametrize("njobs", [1, fc.CR_MAX_JOBS, fc.CR_MAX_JOBS + 1])
def test_col_reduce_multi(njobs):
    """1, 40 (a full job table) and 41 (two launches) jobs of mixed R, C and output dtype: each result within
    the fp64 bound and bitwise the single-job launch's."""
    jobs = fc.col_reduce_jobs(njobs, seed=njobs)
    parts = [_dev(fc.standard((R, C), "crm", i, njobs)) for i, (R, C, _) in enumerate(jobs)]
    outs = [torch.empty(C, device=DEV, dtype=torch.bfloat16 if bf else torch.float32) for _, C, bf in jobs]
    fx().col_reduce_multi(parts, outs)
    for i, ((R, C, bf), p, o) in enumerate(zip(jobs, parts, outs)):
        ref = fc.colsum_ref(p)
        _hold(f"job {i} R={R} C={C}", o, ref["out"], ref["M"], fc.K_COLSUM, op="col_reduce")
        _same_bits(f"job {i} vs single launch", o, _reduce_single(p, bf))


@pytest.mark.parametrize("C", fc.CR_CS)
def test_col_reduce_every_round(C):
    """R on both sides of col_reduce's 16-phase and 128-row rounds, fp32 and bf16 outputs."""
    for R in fc.CR_RS:
        p = _dev(fc.standard((R, C), "cr", R, C))
        ref = fc.colsum_ref(p)
        for bf in (False, True):
            _hold(f"R={R} C={C} bf16={bf}", _reduce_single(p, bf), ref["out"], ref["M"], fc.K_COLSUM, op="col_reduce")


@pytest.mark.parametrize("C", fc.CR_CS)
def test_col_reduce_through_ln_bwd(C):
    """R partial rows = ln_bwd's blocks (N = 16 R - 3 rows, odd): dgamma / dbeta within their bounds, and
    ln_bwd_parts + col_reduce_multi give ln_bwd's bits."""
    for R in fc.CR_RS:
        N = 16 * R - 3
        x, _, w, b, dy, _ = _ln_case(N, C, "standard", 1e-5, torch.float32, False)
        _, mean, rstd = fx().ln_fwd(x, w, b, 1e-5)
        dx, dw, db = fx().ln_bwd(dy, x, w, mean, rstd)
        bw = fc.ln_bwd_ref(dy, x, w, mean, rstd)
        _hold(f"R={R} dgamma", dw, bw["dw"], bw["Mdw"], fc.K_LN_DW, op="ln_dw")
        _hold(f"R={R} dbeta", db, bw["db"], bw["Mdb"], fc.K_LN_DB, op="ln_db")
        dx2, pdw, pdb = fx().ln_bwd_parts(dy, x, w, mean, rstd, None)
        assert pdw.shape == (R, C)
        _same_bits("dx", dx2, dx)
        _same_bits("dgamma", _reduce_single(pdw), dw)
        _same_bits("dbeta", _reduce_single(pdb), db)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", fc.CR_CS)
def test_col_reduce_through_bias_gelu_bwd_and_column_sum(C, dtype):
    """R partial rows = the row splits S = ceil(N / 32) <= 128 (N = 32 R - 5)."""
    for R in [r for r in fc.CR_RS if r <= 128]:
        N = 32 * R - 5
        x = _dev(fc.standard((N, C), "cgx", R, C), dtype)
        dy = _dev(fc.standard((N, C), "cgd", R, C), dtype)
        b = _dev(torch.randn(C, generator=fc._gen("cgb", C)))
        assert fx().colsum_splits(N) == R
        dx, db = fx().bias_gelu_bwd(dy, x, b)
        ref = fc.gelu_ref(x, b, dy)
        _hold(f"R={R} gelu db", db, ref["db"], ref["Mdb"], fc.K_GELU_DB, ref["Xdb"], op="gelu_db")
        dx2, pdb = fx().bias_gelu_bwd_parts(dy, x, b)
        _same_bits("dx", dx2, dx)
        _same_bits("db", _reduce_single(pdb), db)
        cs = fc.colsum_ref(dy)
        for bf in (False, True):
            got = fx().column_sum(dy, bf)
            _hold(f"R={R} column_sum bf16={bf}", got, cs["out"], cs["M"], fc.K_COLSUM, op="column_sum")
            _same_bits("column_sum", _reduce_single(fx().column_sum_parts(dy), bf), got)


@pytest.mark.parametrize("njobs", [fc.CS_MAX_JOBS, fc.CS_MAX_JOBS + 1])
def test_column_sum_parts_multi(njobs):
    """64 (a full job table) and 65 (two launches) bf16 activations: the partials are bitwise column_sum_parts'."""
    shapes = [(32 * fc.CR_RS[i % 6] - 5 - i % 3, (8, 24, 40, 520)[i % 4]) for i in range(njobs)]
    xs = [_dev(fc.standard(s, "cspm", i), torch.bfloat16) for i, s in enumerate(shapes)]
    parts = [torch.full((fx().colsum_splits(N), H), math.nan, device=DEV) for N, H in shapes]
    fx().column_sum_parts_multi(xs, parts)
    for i, (x, p) in enumerate(zip(xs, parts)):
        _same_bits(f"job {i}", p, fx().column_sum_parts(x))
    cs = fc.colsum_ref(xs[-1])
    _hold("last job", _reduce_single(parts[-1]), cs["out"], cs["M"], fc.K_COLSUM, op="column_sum")


# ----------------------------------------------------------------------------
# bias + GELU
# ----------------------------------------------------------------------------
def _gelu_check(label, x, b, dy):
    y = fx().bias_gelu_fwd(x, b)
    ref = fc.gelu_ref(x, b, dy)
    _hold(f"{label} y", y, ref["y"], ref["My"], fc.K_GELU_Y, ref["Xy"], op="gelu_y")
    if dy is None:
        return y, None, None
    dx, db = fx().bias_gelu_bwd(dy, x, b)
    _hold(f"{label} dx", dx, ref["dx"], ref["Mdx"], fc.K_GELU_DX, ref["Xdx"], op="gelu_dx")
    _hold(f"{label} db", db, ref["db"], ref["Mdb"], fc.K_GELU_DB, ref["Xdb"], op="gelu_db")
    return y, dx, db


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", fc.GELU_HS)
def test_bias_gelu(H, dtype):
    b = _dev(torch.randn(H, generator=fc._gen("gb", H)))
    for N in fc.GELU_NS:
        x = _dev(fc.standard((N, H), "gx", N, H), dtype)
        dy = _dev(fc.standard((N, H), "gdy", N, H), dtype)
        y, dx, db = _gelu_check(f"gelu N={N} H={H}", x, b, dy)
        if N in (5, 33):  # ops.bias_gelu and its autograd: the bindings' bits
            xa, ba = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
            y2 = ops.bias_gelu(xa, ba)
            y2.backward(dy)
            _same_bits("ops y", y2.detach(), y)
            _same_bits("ops dx", xa.grad, dx)
            _same_bits("ops db", ba.grad, db)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bias_gelu_tail(dtype):
    """A dense grid over [-9, 9]: in the negative tail 1 + erf cancels, y -> -0 and the bound is |z| u.
    +-0, +-1e20 and +-inf (forward only) are exact: 0.5 z (1 + erf) = z, -0 or, at -inf, NaN as torch."""
    x = _dev(fc.gelu_tail(8), dtype)
    b = torch.zeros(8, device=DEV)
    dy = _dev(fc.standard(tuple(x.shape), "tdy"), dtype)
    _gelu_check("gelu tail", x, b, dy)
    sp = _dev(torch.tensor(fc.GELU_SPECIALS + (1.0, -1.0)).view(1, 8), dtype)
    y = fx().bias_gelu_fwd(sp, b).float()[0]
    want = fc.gelu_ref(sp, b)["y"][0]
    assert torch.isnan(y).tolist() == [False] * 5 + [True, False, False], y
    assert torch.equal(y[:5].double(), want[:5]) and float(y[4]) == math.inf and float(y[2]) == float(sp[0, 2]), y


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H", [fc.GELU_CHUNK2, fc.GELU_SWEEP3])
def test_bias_gelu_fwd_second_chunk_and_sweep(N, H, dtype):
    """Forward only, above 2048 x 256 vectors (the second chunk of an iteration is a chunk of its own) and
    above twice that (a second iteration).  The reference is evaluated in slices of 2^17 rows."""
    b = _dev(torch.randn(H, generator=fc._gen("gb", H)))
    x = _dev(fc.standard((N, H), "gbig", N), dtype)
    y = fx().bias_gelu_fwd(x, b)
    step = 1 << 17
    for lo in range(0, N, step):
        ref = fc.gelu_ref(x[lo:lo + step], b)
        _hold(f"gelu N={N} rows {lo}..", y[lo:lo + step], ref["y"], ref["My"], fc.K_GELU_Y, ref["Xy"], op="gelu_y")


# ----------------------------------------------------------------------------
# softmax cross-entropy
# ----------------------------------------------------------------------------
GS = 3.0


def _xent_check(label, z, y, bad_rows=None, bad_labels=None):
    """Forward and backward through the bindings (lse and the per-row loss are hidden by ops.softmax_xent),
    then ops.softmax_xent and its autograd: the same dz bits, the mean loss within the rows' bounds.
    ``bad_rows``: rows whose lse, loss and dz must be NaN; ``bad_labels``: rows whose loss and dz must be NaN."""
    N, K = z.shape
    none = torch.zeros(N, dtype=torch.bool, device=DEV)
    bad_rows = none if bad_rows is None else bad_rows.to(DEV)
    bad_labels = none if bad_labels is None else bad_labels.to(DEV)
    nan_loss = bad_rows | bad_labels
    loss, lse = fx().xent_fwd(z, y)
    ref = fc.xent_fwd_ref(z, y)
    assert torch.equal(torch.isnan(ref["lse"]), bad_rows) and torch.equal(torch.isnan(ref["loss"]), nan_loss), label
    assert torch.equal(torch.isnan(lse), bad_rows), f"{label}: NaN pattern of lse {torch.isnan(lse).tolist()}"
    assert torch.equal(torch.isnan(loss), nan_loss), f"{label}: NaN pattern of the row loss {torch.isnan(loss).tolist()}"
    _hold(f"{label} lse", lse, ref["lse"], ref["Mlse"], fc.K_XENT_LSE, where=~bad_rows, op="xent_lse")
    _hold(f"{label} loss", loss, ref["loss"], ref["Mloss"], fc.K_XENT_LOSS, where=~nan_loss, op="xent_loss")
    dz = fx().xent_bwd(z, y, lse, torch.tensor([GS], device=DEV))
    bw = fc.xent_bwd_ref(z, y, lse, GS)
    assert torch.equal(torch.isnan(dz.float()).all(-1), nan_loss), f"{label}: NaN rows of dz"
    assert torch.equal(torch.isnan(dz.float()).any(-1), nan_loss), f"{label}: NaN elements of dz off the NaN rows"
    _hold(f"{label} dz", dz, bw["dz"], bw["Mdz"], fc.K_XENT_DZ, where=~nan_loss.view(-1, 1), op="xent_dz")
    za = z.clone().requires_grad_(True)
    mean = ops.softmax_xent(za, y)
    (GS * mean).backward()
    assert mean.dtype == torch.float32
    _same_bits(f"{label} ops dz", za.grad, dz)
    if bool(nan_loss.any()):
        assert bool(torch.isnan(mean)), f"{label}: mean loss {float(mean)} with a NaN row"
    else:
        # mean of N fp32 row losses: the rows' own bounds, plus N - 1 additions and a division of at most
        # u sum|loss| each
        E = fc.bound(fc.K_XENT_LOSS, ref["Mloss"]).mean() + N * fc.EPS24 * ref["loss"].abs().mean()
        assert abs(float(mean) - float(ref["loss"].mean())) <= float(E), (label, float(mean), float(ref["loss"].mean()))
    return dz


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", fc.XENT_KS)
def test_softmax_xent(K, dtype):
    bf = dtype == torch.bfloat16
    for N in fc.XENT_NS:
        for fam in fc.XENT_FAMILIES:
            z = _dev(fc.act(fc.xent_logits(fam, N, K), bf), dtype)
            _xent_check(f"xent N={N} K={K} {fam}", z, fc.xent_labels(N, K).to(DEV))


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_xent_bwd_grid_stride(dtype):
    N, K = fc.XENT_BWD_STRIDE
    _xent_check("xent stride", _dev(fc.xent_logits("standard", N, K), dtype), fc.xent_labels(N, K).to(DEV))


_MASKED = fc.masked_cases()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(_MASKED)), ids=[c[0] for c in _MASKED])
def test_softmax_xent_masked_logits(case, dtype):
    """-inf logits are probability 0: finite lse / loss, dz == 0 there (lane_first: the first logit of a lane
    is -inf and a finite one follows 64 columns later; but_label: only the label's logit is finite, loss 0)."""
    name, z, y = _MASKED[case]
    z = _dev(z, dtype)
    dz = _xent_check(f"xent masked {name}", z, y.to(DEV))
    assert bool((dz[torch.isinf(z)] == 0).all())
    if name.startswith("but_label"):
        loss, _ = fx().xent_fwd(z, y.to(DEV))
        assert bool((loss == 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_softmax_xent_all_masked_row_is_nan(dtype):
    z, y, bad = fc.all_inf_case()
    _xent_check("xent all -inf", _dev(z, dtype), y.to(DEV), bad_rows=bad)


_NAN = fc.nan_logit_cases()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", range(len(_NAN)), ids=[c[0] for c in _NAN])
def test_softmax_xent_nan_logit(case, dtype):
    """One NaN logit (every lane position at K = 10; first or later element of a lane at K = 129), never the
    label's own: that row's lse, loss and dz are NaN, the mean loss is NaN, the clean rows stay within bounds."""
    name, z, y, bad = _NAN[case]
    _xent_check(f"xent nan_logit {name}", _dev(z, dtype), y.to(DEV), bad_rows=bad)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lab", fc.BAD_LABELS)
@pytest.mark.parametrize("K", [10, 129])
def test_softmax_xent_label_out_of_range(K, lab, dtype):
    """Labels K, -1 and -100 (torch's ignore_index is not supported): NaN row loss, NaN mean loss, NaN dz row;
    the other rows' lse, loss and dz stay correct."""
    N = 5
    y = fc.xent_labels(N, K)
    y[3] = K if lab == "K" else lab
    bad = torch.arange(N) == 3
    _xent_check(f"xent label {lab}", _dev(fc.xent_logits("standard", N, K), dtype), y.to(DEV), bad_labels=bad)


# ----------------------------------------------------------------------------
# determinism
# ----------------------------------------------------------------------------
def test_backward_passes_are_deterministic():
    """Two runs of each backward are bitwise equal (no float atomics anywhere)."""
    for dtype in DTYPES:
        x, r, w, b, dy, gs = _ln_case(16401, 24, "standard", 1e-5, dtype, True)
        y, mean, rstd, s = fx().ln_fwd(x, w, b, 1e-5, r)
        for a, c in zip(fx().ln_bwd(dy, s, w, mean, rstd, gs), fx().ln_bwd(dy, s, w, mean, rstd, gs)):
            _same_bits("ln_bwd", a, c)
        for a, c in zip(fx().bias_gelu_bwd(dy, x, w), fx().bias_gelu_bwd(dy, x, w)):
            _same_bits("bias_gelu_bwd", a, c)
        _same_bits("column_sum", fx().column_sum(dy), fx().column_sum(dy))
        z = _dev(fc.xent_logits("standard", 525, 1000), dtype)
        lab = fc.xent_labels(525, 1000).to(DEV)
        _, lse = fx().xent_fwd(z, lab)
        g = torch.tensor([GS], device=DEV)
        _same_bits("xent_bwd", fx().xent_bwd(z, lab, lse, g), fx().xent_bwd(z, lab, lse, g))
    dh = _dev(fc.standard((17, 6, 64), "dh"), torch.bfloat16)
    for a, c in zip(fx().embed_tokens_bwd(dh), fx().embed_tokens_bwd(dh)):
        _same_bits("embed_tokens_bwd", a, c)


# ----------------------------------------------------------------------------
# exact (bitwise) ops
# ----------------------------------------------------------------------------
def _seq_sum_bf16(parts):
    """Sequential fp32 sum over dim 0 (IEEE float32 additions in torch), then RNE to bf16."""
    acc = torch.zeros(parts.shape[1:], device=parts.device)
    for s in range(parts.shape[0]):
        acc = acc + parts[s].float()
    return acc.to(torch.bfloat16)


@pytest.mark.parametrize("S,n", [(S, n) for S in fc.SPLIT_S for n in fc.SPLIT_N] + [(2, fc.SPLIT_STRIDE_N)])
def test_split_sum_bf16_is_the_sequential_fp32_sum(S, n):
    parts = _dev(fc.standard((S, n), "split", S, n % 9973), torch.bfloat16)
    _same_bits(f"split_sum S={S} n={n}", fx().split_sum_bf16(parts), _seq_sum_bf16(parts))


@pytest.mark.parametrize("N,D", fc.EMBED_ND)
@pytest.mark.parametrize("B", fc.EMBED_B)
def test_embed_tokens_exact(B, N, D):
    """Forward: one fp32 add, one rounding.  Backward: dy a bitwise copy of dh[:, 1:], dpos the sequential fp32
    sum over b rounded once, dcls == dpos[0]."""
    y = _dev(fc.standard((B, N, D), "ey", B), torch.bfloat16)
    cls = _dev(fc.standard((D,), "ec", B) * 0.02, torch.bfloat16)
    pos = _dev(fc.standard((N + 1, D), "ep", B) * 0.02, torch.bfloat16)
    h = fx().embed_tokens_fwd(y, cls, pos)
    want = (torch.cat([cls.view(1, 1, D).expand(B, 1, D), y], 1).float() + pos.float()).to(torch.bfloat16)
    _same_bits("embed fwd", h, want)
    _same_bits("ops.embed_tokens", ops.embed_tokens(y, cls.view(1, 1, D), pos.view(1, N + 1, D)), want)
    dh = _dev(fc.standard((B, N + 1, D), "edh", B), torch.bfloat16)
    dy, dpos, dcls = fx().embed_tokens_bwd(dh)
    _same_bits("dy", dy, dh[:, 1:].contiguous())
    _same_bits("dpos", dpos, _seq_sum_bf16(dh))
    _same_bits("dcls", dcls, dpos[0].contiguous())


@pytest.mark.parametrize("C,P", fc.PATCH_LAYOUTS)
def test_patchify_u8_every_byte_in_every_position(C, P):
    """All 256 byte values in all 8 positions of the kernel's pixel vectors, H != W: bitwise float(v) * (1 / 255f)
    rounded to bf16; within 1 bf16 ulp of float64 v / 255 rounded to bf16, with exactly the number of
    mismatches the emulation of that product predicts."""
    x = fc.patch_image(C, P)
    got = ops.patchify_u8(x.to(DEV), P).cpu()
    emu, ref = fc.patchify_emu(x, P), fc.patchify_ref(x, P)
    _same_bits("patchify", got, emu)
    ref_bf = ref.to(torch.bfloat16)  # float64 -> bf16 in one rounding
    ulp = (got.view(torch.int16).int() - ref_bf.view(torch.int16).int()).abs()  # same sign: the bit patterns are ordered
    assert int(ulp.max()) <= 1
    assert int((ulp != 0).sum()) == int((emu.view(torch.int16) != ref_bf.view(torch.int16)).sum())


def _copy_regions(sizes, seed):
    srcs, bufs, dsts = [], [], []
    for i, nb in enumerate(sizes):
        n = nb // 4
        srcs.append(torch.randint(-2**31, 2**31 - 1, (n,), generator=fc._gen("copy", seed, i), dtype=torch.int32).to(DEV))
        buf = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)  # 8 guard words behind the region
        bufs.append(buf)
        dsts.append(buf[:n])
    return srcs, bufs, dsts


@pytest.mark.parametrize("sizes", [
    (4,), (16,), (fc.COPY_BIG,), (12, 4096 + 4), (4, 8, 12, 16, 20, 24, 28, 32, 4096, 4096 + 8, 65536 + 12, 48),
], ids=["4B", "16B", "big", "two", "twelve"])
def test_multi_copy(sizes):
    """1, 2 and 12 regions, byte sizes with % 16 in {0, 4, 8, 12}, below 16, and one above the 8 MB a sweep of
    the grid covers: exact copies, the guard words behind every destination untouched."""
    assert len(sizes) <= fc.COPY_MAX
    srcs, bufs, dsts = _copy_regions(sizes, len(sizes))
    fx().multi_copy(dsts, srcs)
    for nb, s, buf in zip(sizes, srcs, bufs):
        n = nb // 4
        assert torch.equal(buf[:n], s), f"region of {nb} bytes"
        assert bool((buf[n:] == 0x5A5A5A5A).all()), f"guard words behind the region of {nb} bytes"


def test_multi_copy_refuses_13_regions():
    srcs, bufs, dsts = _copy_regions((16,) * (fc.COPY_MAX + 1), 13)
    with pytest.raises(RuntimeError):
        fx().multi_copy(dsts, srcs)
    torch.cuda.synchronize()
    assert all(bool((b == 0x5A5A5A5A).all()) for b in bufs)
