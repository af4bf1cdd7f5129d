"""csrc/optim.hip against an fp64 reference, every Adam / SGD path (MI355X only).

The four kernels (``adam_kernel``, ``sgd_kernel``, ``adam_mt_kernel<FD>``, ``sgd_mt_kernel<FD>``),
the three data paths of the multi-tensor ones (dense float4 + scalar tail, channels-last staged
through LDS, channels-last gather / scatter), both index-math arms (``P2_MT_FASTDIV``) and both ways
of receiving per-step data (gradient list + host bias corrections, persistent ``gtab`` + device-side
``t_dev`` corrections) are held, element by element and output by output, to

    |got - ref| <= K 2^-24 M + FLOOR

``ref`` is the float64 single-step reference of tests/optim_cases.py (anchored to float64 torch.optim
by tests/test_optim_reference.py), evaluated on the hyperparameters as the kernels receive them
(through float32), for a *given* state and step t -- not a trajectory from zero.  M is the magnitude of
the terms summed into the element, FLOOR = 2^-126 is the float32 normal limit (a format limit, not a
tolerance).  On poisoned elements (a NaN / +Inf gradient) finiteness is compared instead.  The
cases, value families (wide, fresh, tiny, large, poison), hyperparameter sets and the multi-tensor
layout (every shape with a bf16 and with an fp32 gradient, ~200 k elements) live in optim_cases.py.

K: emulated, not fitted
-----------------------
A float32 emulation of the kernels' rounding points (explicit fmaf always fused; the three a * b + c
the compiler may contract in both forms), 2^17 elements per case, every hyperparameter set, every
t in {1, 2, 10, 1000, 100000}; largest |emu - ref| / (2^-24 M) per family:

    family   Adam p   Adam m   Adam v   SGD p   SGD buf
    wide      6.02     2.16     4.00    2.41     1.72
    fresh     5.16     1.68     3.70    2.37     0.99
    tiny      4.73     1.87     3.81    1.00     1.00
    large     4.88     0.95     1.93    1.72     0.00

K = 2 x the largest, rounded up (the 2 covers the compiler's choice of contraction and the ~1 ulp
device sqrtf and divide): K_P = 13, K_M = 5, K_V = 8 for Adam, K_P_SGD = 5, K_BUF = 4 for SGD.
Measured on the MI355X (largest err / (2^-24 M) over this file): Adam p 4.96, m 2.47, v 4.46; SGD
p 2.62, buf 1.92; the t_dev path p 4.24 (0.32 of its widened bound, which uses c = 3: 2 for powf
plus 1 for rsqrtf, not fitted).

Host bias corrections (the fix that came with this file)
--------------------------------------------------------
The kernels accumulate m and v with the float32 betas; csrc/bindings.cpp computed step_size and
inv_sqrt_bc2 from the unrounded doubles (v_hat = g^2 (1 - 1.3e-5) at t = 1).  It now computes them
from the float32 lr and betas, as the t_dev path and the reference do.  Emulated (CPU, wide family,
not measured) largest p error in units of 2^-24 M_p:

    t         before    after
    1         116.33     4.77
    2         116.48     6.02
    10        113.78     5.60
    1000       67.96     5.30
    100000      4.54     4.54

Measured regression check: with the fix reverted, 29 of the 67 tests here fail on the MI355X -- every
host-path Adam case (test_adam_step at every n, test_adam_mt_step at t = 1, 2 and 1000, and the Adam
cases of the shadow, skip, poison, gtab, path and chained tests), largest observed ratio 116.28 x
2^-24 M_p against K_P = 13.  The t_dev tests and all of SGD pass either way.

Measured bitwise claims (MI355X)
--------------------------------
* dense vs LDS-staged vs gather path on the same element values (Adam coupled and decoupled, SGD
  Nesterov and dampened, bf16 and fp32 gradients): 0 elements of p, m, v / buf differ -- asserted.
* ``P2_MT_FASTDIV=0`` (child process) vs the default arm, whole layout, every hyperparameter set:
  bitwise equal in p, state and shadow -- asserted.
* ``gtab`` (with 0 entries for skipped tensors, ``grads=[]``) vs the gradient list: bitwise equal --
  asserted.
* whole-arena kernel on a flat fp32 arena vs multi-tensor kernel on the same values as one dense
  tensor with an fp32 gradient (n = 1028; Adam coupled and decoupled, SGD Nesterov): p, state and
  shadow bitwise equal -- asserted (both traversals instantiate the same AdamRule / SgdRule).
* ``p_bf16=None`` vs a shadow: same p and state bits; the shadow is the kernel's own p rounded to bf16,
  bitwise, at its channels-last positions; padding, unshadowed and skipped regions keep their sentinels.

What the bounds see
-------------------
Arithmetic-only mutations of csrc/optim.hip (none moves an address; never committed), number of
the 67 tests here that fail:

    eps moved inside the bias correction ((sqrt(v) + eps) * inv_sqrt_bc2)      34
    (1 - dampening) dropped                                                     8
    Nesterov reading the old buffer                                            10
    decoupled decay applied after the update                                   16
    inv_sqrt_bc2 replaced by 1 at t = 1000                                      4
    (host bias corrections from the double betas, above)                       29

Memory: the largest n (2048 * 1024 + 1028: the grid is capped at 2048 blocks of 256 float4 threads,
so the grid-stride loop runs a partly filled second sweep) makes four fp32 arenas plus the shadow 38 MB by itself; the float64 reference is therefore
evaluated in slices.  Every other test stays below 20 MB.
"""

from __future__ import annotations

import functools
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import optim_cases as oc  # noqa: E402
from p2pfl_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NS = (4, 64, 1028, 2048 * 1024 + 1028)  # the last: a partly filled second sweep of the grid-stride loop
PLAIN_STEPS = (1, 10, 100000)
MT_STEPS = (1, 2, 1000)
TDEV_STEPS = (1, 2, 3, 10, 1000, 100000)
CHILD_TIMEOUT = 120
CHUNK = 1 << 18


@pytest.fixture(autouse=True)
def _require_ext():
    ops.ext()  # fail loudly if the native extension is missing on a GPU box


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _hold(label, got, ref, M, K, extra=None, poisoned=None, quiet=False):
    """|got - ref| <= K 2^-24 M + FLOOR (+ extra) on every element whose reference is finite;
    on the others (the poisoned ones, and only those) NaN where the reference is NaN and the
    reference's infinity where it is infinite.  Prints and returns the largest err / bound."""
    fin = torch.isfinite(ref)
    if poisoned is None:
        assert bool(fin.all()), f"{label}: the reference is not finite"
    else:
        assert torch.equal(fin, ~poisoned), f"{label}: the reference is non-finite off the poisoned elements"
        bad = ~fin
        assert torch.equal(torch.isnan(got[bad]), torch.isnan(ref[bad])), f"{label}: NaN pattern of the poisoned elements"
        inf = torch.isinf(ref)
        assert torch.equal(got[inf].double(), ref[inf]), f"{label}: infinities of the poisoned elements"
    bound = K * oc.EPS24 * M + oc.FLOOR
    if extra is not None:
        bound = bound + extra
    err = (got.double() - ref).abs()
    r = torch.where(fin, err / bound, torch.zeros_like(err))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)  # a NaN where the reference is finite
    worst = float(r.max()) if r.numel() else 0.0
    if not quiet:
        print(f"{label}: worst err / bound {worst:.3f} (err / (2^-24 M): {worst * K:.2f})")
    if worst > 1.0:
        i = int(r.argmax())
        pytest.fail(f"{label}: element {i}: got {float(got[i])!r} ref {float(ref[i])!r} err {float(err[i]):.3e} "
                    f"bound {float(bound[i]):.3e} ({worst * K:.2f} x 2^-24 M); {int((r > 1).sum())} elements outside",
                    pytrace=False)
    return worst


def _same_bits(label, got, want, where=None):
    a, b = _bits(got), _bits(want)
    if where is not None:
        a, b = a[where], b[where]
    n = int((a != b).sum())
    assert n == 0, f"{label}: {n} elements differ bitwise"


def _shadow_ok(label, shadow, want):
    """Bitwise where the wanted bf16 value is finite; non-finite of the same kind elsewhere."""
    fin = torch.isfinite(want.float())
    _same_bits(label, shadow, want, fin)
    assert torch.equal(torch.isnan(shadow.float()[~fin]), torch.isnan(want.float()[~fin])), label
    assert not bool(torch.isfinite(shadow.float()[~fin]).any()), label


# ----------------------------------------------------------------------------
# plain kernels
# ----------------------------------------------------------------------------
def _hold_plain(label, x, got, ref_fn, todo):
    """_hold in slices of 2^18 elements (the inputs ``x`` stay on the CPU), so the float64 reference
    of the largest n does not sit in device memory next to the arenas."""
    n = got["p"].numel()
    worst = {k: 0.0 for k, _, _ in todo}
    for lo in range(0, n, CHUNK):
        sl = slice(lo, min(n, lo + CHUNK))
        ref = ref_fn({k: t[sl].to(DEV) for k, t in x.items()})
        for k, Mk, K in todo:
            worst[k] = max(worst[k], _hold(f"{label} {k} [{lo}:]", got[k][sl], ref[k], ref[Mk], K, quiet=True))
    for k, _, K in todo:
        print(f"{label} {k}: worst err / bound {worst[k]:.3f} (err / (2^-24 M): {worst[k] * K:.2f})")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", list(oc.ADAM_SETS))
def test_adam_step(name, n):
    hp = oc.ADAM_SETS[name]
    todo = [("p", "Mp", oc.K_P), ("m", "Mm", oc.K_M), ("v", "Mv", oc.K_V)]
    for fam in oc.FAMILIES:
        x = oc.family(fam, n)
        g = x["g"].to(DEV)
        for t in oc.family_steps(fam, PLAIN_STEPS):
            got = {k: x[k].to(DEV) for k in "pmv"}
            shadow = torch.full((n,), oc.SENTINEL["shadow"], dtype=torch.bfloat16, device=DEV)
            ops.adam_step(got["p"], g, got["m"], got["v"], step=t, p_bf16=shadow, **hp)
            _hold_plain(f"adam_step {name} n={n} {fam} t={t}", x, got,
                        lambda c: oc.adam_ref(c["p"], c["g"], c["m"], c["v"], t, hp), todo)
            _same_bits("shadow", shadow, got["p"].to(torch.bfloat16))
            del shadow
            if fam == "wide" and t == 10:  # once without the shadow: the same bits
                two = {k: x[k].to(DEV) for k in "pmv"}
                ops.adam_step(two["p"], g, two["m"], two["v"], step=t, p_bf16=None, **hp)
                for k in "pmv":
                    _same_bits("p_bf16=None", two[k], got[k])
                del two


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("name", list(oc.SGD_SETS))
def test_sgd_step(name, n):
    hp = oc.SGD_SETS[name]
    todo = [("p", "Mp", oc.K_P_SGD)] + ([("buf", "Mb", oc.K_BUF)] if hp["has_buf"] else [])
    for fam in oc.FAMILIES:
        x = oc.family(fam, n)
        g = x["g"].to(DEV)
        got = dict(p=x["p"].to(DEV), buf=x["buf"].to(DEV) if hp["has_buf"] else None)
        shadow = torch.full((n,), oc.SENTINEL["shadow"], dtype=torch.bfloat16, device=DEV)
        ops.sgd_step(got["p"], g, got["buf"], p_bf16=shadow, **oc.sgd_kwargs(hp))
        _hold_plain(f"sgd_step {name} n={n} {fam}", x, got,
                    lambda c: oc.sgd_ref(c["p"], c["g"], c["buf"] if hp["has_buf"] else None, hp), todo)
        _same_bits("shadow", shadow, got["p"].to(torch.bfloat16))
        del shadow
        if fam == "wide":
            two = dict(p=x["p"].to(DEV), buf=x["buf"].to(DEV) if hp["has_buf"] else None)
            ops.sgd_step(two["p"], g, two["buf"], p_bf16=None, **oc.sgd_kwargs(hp))
            _same_bits("p_bf16=None", two["p"], got["p"])
            if hp["has_buf"]:
                _same_bits("p_bf16=None", two["buf"], got["buf"])
            del two


# ----------------------------------------------------------------------------
# multi-tensor kernels
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layout():
    return oc.mt_layout_cases().to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(seed=0, poison=False):
    return oc.mt_inputs(_layout(), "wide", seed=seed, poison=poison)


def _sets(opt):
    return oc.ADAM_SETS if opt == "adam" else oc.SGD_SETS


def _skip_ids(lay):
    return tuple(lay.index(s, bf) for s in oc.SKIP for bf in (True, False))


def _check_mt(label, lay, opt, hp, t, inp, out, *, skipped=(), widen=False):
    """Every arena after one multi-tensor launch: padding and skipped tensors bitwise
    untouched, every other element within the bound of the fp64 reference at step t, the
    shadow the kernel's own p at its channels-last positions."""
    untouched = lay.padding_mask()
    for i in skipped:
        off, n, _ = lay.table[i]
        untouched[off:off + n] = True
    untouched = untouched.to(DEV)
    act = ~untouched
    x = {k: inp[k].to(DEV) for k in ("p", "m", "v", "buf", "glog", "poisoned")}
    bad = x["poisoned"][act] if bool(x["poisoned"].any()) else None
    if opt == "adam":
        ref = oc.adam_ref(x["p"], x["glog"], x["m"], x["v"], t, hp)
        todo = [("p", "Mp", oc.K_P), ("m", "Mm", oc.K_M), ("v", "Mv", oc.K_V)]
    else:
        ref = oc.sgd_ref(x["p"], x["glog"], x["buf"] if hp["has_buf"] else None, hp)
        todo = [("p", "Mp", oc.K_P_SGD)] + ([("buf", "Mb", oc.K_BUF)] if hp["has_buf"] else [])
    worst = {}
    for k, Mk, K in todo:
        _same_bits(f"{label}: {k} padding / skipped tensors", out[k], x[k], untouched)
        extra = oc.tdev_widening(t, hp, ref)[act] if widen and k == "p" else None
        worst[k] = _hold(f"{label} {k}", out[k][act], ref[k][act], ref[Mk][act], K, extra=extra, poisoned=bad)
    if out["shadow"] is not None:
        _shadow_ok(f"{label}: shadow", out["shadow"], oc.expected_shadow(lay, out["p"], out["shadow0"], skipped))
    return worst


@pytest.mark.parametrize("t", MT_STEPS)
@pytest.mark.parametrize("name", list(oc.ADAM_SETS))
def test_adam_mt_step(name, t):
    lay, hp = _layout(), oc.ADAM_SETS[name]
    out = oc.run_mt(ops, lay, "adam", hp, t, _inputs(), DEV)
    _check_mt(f"adam_mt {name} t={t}", lay, "adam", hp, t, _inputs(), out)


@pytest.mark.parametrize("name", list(oc.SGD_SETS))
def test_sgd_mt_step(name):
    lay, hp = _layout(), oc.SGD_SETS[name]
    out = oc.run_mt(ops, lay, "sgd", hp, 1, _inputs(), DEV)
    _check_mt(f"sgd_mt {name}", lay, "sgd", hp, 1, _inputs(), out)


@pytest.mark.parametrize("opt,name", [("adam", "adam_wd"), ("sgd", "nesterov"), ("sgd", "plain")])
def test_mt_without_shadow(opt, name):
    lay, hp = _layout(), _sets(opt)[name]
    out = oc.run_mt(ops, lay, opt, hp, 2, _inputs(), DEV, shadow=False)
    _check_mt(f"{opt}_mt {name} p_bf16=None", lay, opt, hp, 2, _inputs(), out)


@pytest.mark.parametrize("opt,name", [("adam", "adamw"), ("sgd", "damp"), ("sgd", "plain")])
def test_mt_skipped_tensors(opt, name):
    """A None gradient for one dense, one staged and one gather tensor (each with a bf16 and with an
    fp32 gradient): their p, state and shadow stay bitwise as they were, everything else is updated."""
    lay, hp = _layout(), _sets(opt)[name]
    skipped = _skip_ids(lay)
    out = oc.run_mt(ops, lay, opt, hp, 2, _inputs(), DEV, skipped=skipped)
    _check_mt(f"{opt}_mt {name} skipped", lay, opt, hp, 2, _inputs(), out, skipped=skipped)


@pytest.mark.parametrize("opt,name", [("adam", "adam_wd"), ("adam", "adamw"), ("sgd", "nesterov"), ("sgd", "damp"),
                                      ("sgd", "plain")])
def test_mt_poison(opt, name):
    """A NaN / +Inf gradient element poisons its own element only: every other element of the same
    LDS-staged chunk, gather chunk and dense tail is finite and within the bound."""
    lay, hp = _layout(), _sets(opt)[name]
    inp = _inputs(poison=True)
    out = oc.run_mt(ops, lay, opt, hp, 2, inp, DEV)
    _check_mt(f"{opt}_mt {name} poison", lay, opt, hp, 2, inp, out)


@pytest.mark.parametrize("opt,name", [("adam", "adam_wd"), ("sgd", "nesterov")])
def test_gtab_is_bitwise_the_gradient_list(opt, name):
    """The same gradients through a persistent device table of addresses (0 = skipped) and grads=[]."""
    lay, hp = _layout(), _sets(opt)[name]
    skipped = _skip_ids(lay)[:3]
    a = oc.run_mt(ops, lay, opt, hp, 2, _inputs(), DEV, skipped=skipped)
    b = oc.run_mt(ops, lay, opt, hp, 2, _inputs(), DEV, skipped=skipped, via="gtab")
    for k in a:
        if a[k] is not None:
            _same_bits(f"gtab vs list: {k}", b[k], a[k])
    _check_mt(f"{opt}_mt {name} gtab", lay, opt, hp, 2, _inputs(), b, skipped=skipped)


@pytest.mark.parametrize("t", TDEV_STEPS)
def test_adam_mt_t_dev(t):
    """Device-side bias corrections: t comes from t_dev (the step argument is 1 on purpose), the
    result is held to the fp64 reference at t, p widened by the cancellation term of 1 - powf(b, t)."""
    lay = _layout()
    for name, hp in oc.ADAM_SETS.items():
        out = oc.run_mt(ops, lay, "adam", hp, t, _inputs(), DEV, via="gtab", t_dev=t, step=1)
        _check_mt(f"adam_mt {name} t_dev={t}", lay, "adam", hp, t, _inputs(), out, widen=True)


def test_fastdiv_arms_are_bitwise_equal(tmp_path):
    """P2_MT_FASTDIV=0 (index by integer division) in a fresh child process: only addresses differ
    between the arms, so every arena must come out bit for bit as in this process."""
    assert os.environ.get("P2_MT_FASTDIV", "1") != "0", "the parent must run the default arm"
    base = oc.run_fastdiv_cases(ops, DEV)
    env = dict(os.environ, P2_MT_FASTDIV="0")
    out = str(tmp_path / "fastdiv0.pt")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "optim_fastdiv_worker.py"), out], cwd=ROOT,
                           env=env, timeout=CHILD_TIMEOUT, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.fail(f"worker still running after {CHILD_TIMEOUT} s", pytrace=False)
    if r.returncode != 0:
        pytest.fail(f"worker exited {r.returncode}\n{r.stderr[-2000:]}", pytrace=False)
    child = torch.load(out)
    assert set(child) == set(base) and len(base) == len(oc.FASTDIV_CASES)
    for case, res in base.items():
        assert set(child[case]) == set(res)
        for k, x in res.items():
            _same_bits(f"P2_MT_FASTDIV=0 {case} {k}", child[case][k], x)


@pytest.mark.parametrize("opt,name", [("adam", "adam_wd"), ("adam", "adamw"), ("sgd", "nesterov"), ("sgd", "damp")])
def test_paths_are_bitwise_equal(opt, name):
    """The same element values as a dense tensor, a channels-last tensor staged through LDS and a
    channels-last gather tensor (gradient permuted to match): p and state come out bit for bit equal."""
    n = 9216
    shapes = [(n,), (4, 256, 3, 3), (1, 1024, 3, 3)]
    assert [oc.kind_of(s) for s in shapes] == ["dense", "staged", "gather"]
    lay = oc.Layout(shapes * 2, [True] * 3 + [False] * 3, [True] * 6).to(DEV)
    hp = _sets(opt)[name]
    inp = oc.mt_inputs(lay, "wide", seed=5, same=True)
    out = oc.run_mt(ops, lay, opt, hp, 2, inp, DEV)
    _check_mt(f"{opt}_mt {name} paths", lay, opt, hp, 2, inp, out)
    for half in (0, 3):
        o0 = lay.table[half][0]
        for i in (1, 2):
            oi = lay.table[half + i][0]
            for k in ("p", "m", "v", "buf"):
                if out.get(k) is not None:
                    diff = int((_bits(out[k][oi:oi + n]) != _bits(out[k][o0:o0 + n])).sum())
                    print(f"{opt} {name} {'bf16' if half == 0 else 'fp32'} {oc.kind_of(shapes[i])} vs dense, {k}: {diff} differ")
                    assert diff == 0, (k, shapes[i], diff)


@pytest.mark.parametrize("opt,name", [("adam", "adam_wd"), ("adam", "adamw"), ("sgd", "nesterov")])
def test_arena_and_mt_kernels_are_bitwise_equal(opt, name):
    """One update rule under both traversals: the whole-arena kernel on a flat fp32 arena and the
    multi-tensor kernel on the same values as a single dense tensor with an fp32 gradient give
    bit for bit the same p, state and shadow."""
    n = 1028  # 257 float4, no scalar tail
    assert n in NS
    hp, t = _sets(opt)[name], 2
    lay = oc.Layout([(n,)], [False], [True]).to(DEV)
    inp = oc.mt_inputs(lay, "wide", seed=7)
    mt = oc.run_mt(ops, lay, opt, hp, t, inp, DEV)
    _check_mt(f"{opt}_mt {name} single dense tensor", lay, opt, hp, t, inp, mt)
    g = inp["glog"][:n].to(DEV)
    flat = {k: inp[k][:n].to(DEV) for k in (("p", "m", "v") if opt == "adam" else ("p", "buf"))}
    shadow = torch.full((n,), oc.SENTINEL["shadow"], dtype=torch.bfloat16, device=DEV)
    if opt == "adam":
        ops.adam_step(flat["p"], g, flat["m"], flat["v"], step=t, p_bf16=shadow, **hp)
    else:
        assert hp["has_buf"]
        ops.sgd_step(flat["p"], g, flat["buf"], p_bf16=shadow, **oc.sgd_kwargs(hp))
    for k, x in flat.items():
        _same_bits(f"{opt} {name} whole-arena vs multi-tensor: {k}", mt[k][:n], x)
    _same_bits(f"{opt} {name} whole-arena vs multi-tensor: shadow", mt["shadow"][:n], shadow)


@pytest.mark.parametrize("opt,name", [("adam", "adam_wd"), ("sgd", "nesterov")])
def test_chained_steps(opt, name):
    """Three launches in a row; each step's reference starts from the kernel's own previous
    output, so the bound does not compound."""
    lay = _layout()
    state = None
    for t in (1, 2, 3):
        hp = _sets(opt)[name] if opt == "adam" else dict(oc.SGD_SETS[name], first_step=t == 1)
        inp = dict(_inputs(seed=10 + t))
        if state is not None:
            inp.update(state)
        out = oc.run_mt(ops, lay, opt, hp, t, inp, DEV)
        _check_mt(f"{opt}_mt {name} chained step {t}", lay, opt, hp, t, inp, out)
        state = {k: out[k].cpu() for k in ("p", "m", "v", "buf") if out.get(k) is not None}
