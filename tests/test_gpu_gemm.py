"""Hand-written MFMA GEMM (csrc/gemm.hip) vs an fp32 PyTorch reference on the same bf16 operands."""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

from p2pfl_amd import ops
import importlib

gemm_mod = importlib.import_module("p2pfl_amd.ops.gemm")
from p2pfl_amd.ops.variant import A_PANEL, SINGLE_BUF, TILE256

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _require_ext(monkeypatch):
    ops.ext()
    # these tests exercise the hand-written kernels: no per-shape library choice
    monkeypatch.setattr(gemm_mod, "_POLICY", "native")


def _operands(M, N, K, a_kmajor, b_kmajor, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    A = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    B = torch.randn(N, K, device="cuda", generator=g).to(torch.bfloat16)
    a = A if a_kmajor else A.t().contiguous()
    b = B if b_kmajor else B.t().contiguous()
    return a, b


@pytest.mark.parametrize("a_kmajor,b_kmajor", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 192), (200, 136, 200), (6304 // 8, 768, 768), (72, 1000, 96)])
def test_gemm_layouts_vs_fp32(a_kmajor, b_kmajor, M, N, K):
    """Every operand layout; ragged M (row clamping), N (masked stores) and K (zeroed tail)."""
    if not a_kmajor and M % 8:  # refused loudly, by the planner and by the binding
        from p2pfl_amd.ops.gemm import supported

        assert not supported(M, N, K, a_kmajor, b_kmajor)
        a, b = _operands(M + 8 - M % 8, N, K, a_kmajor, b_kmajor, seed=1)
        a = a[:, :M]  # an m-major [K, M] view with M % 8 != 0
        with pytest.raises(RuntimeError):
            ops.ext().gemm(a, b, a_kmajor, b_kmajor, torch.empty(M, N, device="cuda"), None, False, None, None, 1,
                           A_PANEL | SINGLE_BUF)
        return
    a, b = _operands(M, N, K, a_kmajor, b_kmajor, seed=M + N + K)
    out, _ = ops.gemm(a, b, a_kmajor, b_kmajor, out_dtype=torch.float32)
    ref, _ = ops.gemm_reference(a, b, a_kmajor, b_kmajor)
    torch.testing.assert_close(out, ref, atol=2e-3, rtol=1e-4)


def test_gemm_asymmetric_exact_integers():
    """Small integer operands: exact in bf16 and fp32, so any mis-mapped lane/row shows as an exact mismatch."""
    M, N, K = 160, 96, 128
    A = torch.randint(-3, 4, (M, K), device="cuda").to(torch.bfloat16)
    B = (torch.arange(N * K, device="cuda").view(N, K) % 7 - 3).to(torch.bfloat16)  # asymmetric
    for ak, bk in [(True, True), (True, False), (False, True), (False, False)]:
        a = A if ak else A.t().contiguous()
        b = B if bk else B.t().contiguous()
        out, _ = ops.gemm(a, b, ak, bk, out_dtype=torch.float32)
        assert torch.equal(out, A.float() @ B.float().t()), (ak, bk)


@pytest.mark.parametrize("splits", [2, 4, 8])
def test_gemm_split_k(splits):
    M, N, K = 256, 320, 6304  # the weight-gradient shape class: reduction over token rows, ragged K
    a, b = _operands(M, N, K, False, False, seed=splits)
    out, _ = ops.gemm(a, b, False, False, out_dtype=torch.float32, splits=splits)
    ref, _ = ops.gemm_reference(a, b, False, False)
    torch.testing.assert_close(out, ref, atol=5e-3, rtol=1e-4)


def test_wgrad_split_factor_64_on_long_k():
    """1x1-conv weight gradient class (ResNet-50: K = 32768 pixels, 2 tiles): 64 K-slices
    reduced by tile_slab_reduce, vs fp32."""
    M, N, K = 256, 64, 32768
    assert gemm_mod.splits_for(M, N, K) == 64
    a, b = _operands(M, N, K, False, False, seed=64)
    out = gemm_mod._product(a, b, False, False, torch.float32, gemm_mod.splits_for(M, N, K))
    ref, _ = ops.gemm_reference(a, b, False, False)
    torch.testing.assert_close(out, ref, atol=2e-2, rtol=1e-4)


@pytest.mark.parametrize("bias_dtype", [torch.float32, torch.bfloat16])
def test_gemm_epilogue_bias_gelu_residual(bias_dtype):
    M, N, K = 300, 256, 128
    a, b = _operands(M, N, K, True, True, seed=3)
    bias = torch.randn(N, device="cuda").to(bias_dtype)
    res = torch.randn(M, N, device="cuda").to(torch.bfloat16)
    out, z = ops.gemm(a, b, bias=bias, gelu=True, want_z=True, residual=res, out_dtype=torch.float32)
    ref, zref = ops.gemm_reference(a, b, bias=bias, gelu=True, residual=res)
    torch.testing.assert_close(out, ref, atol=2e-3, rtol=1e-4)
    torch.testing.assert_close(z.float(), zref, atol=3e-2, rtol=8e-3)  # z is stored in bf16


# None = the measured plan; then explicit kernel configurations per product ("native:variant:splits"):
# 128 x 128 tile, 256 x 256 ping-pong (32x32x16 / 16x16x32 MFMA), 256 x 128 ping-pong, split-K, stream-K
_PLANS = [None,
          ("native:0:1", "native:0:1", "native:2:3"),
          ("native:2048:1", "native:2048:2", "native:2048:6"),
          ("native:67584:1", "native:2099200:1", "native:4098:6"),
          ("native:2099200:1", "native:133120:24", "native:10:6"),
          ("native:198656:17", "native:2048:1", "native:2048:8")]


@pytest.mark.parametrize("plan", _PLANS)
@pytest.mark.parametrize("gelu", [False, True])
def test_linear_autograd_vs_fp32(gelu, plan):
    """Kernel configurations for the three products (forward / input gradient / weight
    gradient, chosen per product by ops.gemm._plan) against fp32; None = the measured plan."""
    import importlib

    G = importlib.import_module("p2pfl_amd.ops.gemm")  # the module (ops.gemm is the function)
    torch.manual_seed(0)
    x = torch.randn(4, 197, 768, device="cuda").to(torch.bfloat16).requires_grad_()
    w = (torch.randn(512, 768, device="cuda") * 0.03).to(torch.bfloat16).requires_grad_()
    bias = torch.randn(512, device="cuda").requires_grad_()
    if plan is None:
        y = ops.linear_gelu(x, w, bias) if gelu else ops.linear(x, w, bias)
    else:
        y = G._LinearP.apply(x, w, bias, gelu, plan)
    g = torch.randn_like(y)
    y.backward(g)
    xr, wr, br = (t.detach().float().requires_grad_() for t in (x, w, bias))
    yr = F.linear(xr, wr, br)
    if gelu:
        yr = F.gelu(yr)
    yr.backward(g.float())
    torch.testing.assert_close(y.float(), yr, atol=3e-2, rtol=2e-2)
    torch.testing.assert_close(x.grad.float(), xr.grad, atol=3e-2, rtol=2e-2)
    # dW reduces over 788 rows of a bf16 dZ (rounded GELU backward): judge it on its scale
    scale = wr.grad.abs().max().item()
    torch.testing.assert_close(w.grad.float(), wr.grad, atol=1e-2 * scale, rtol=2e-2)
    torch.testing.assert_close(bias.grad, br.grad, atol=1e-1, rtol=2e-2)


def test_vit_block_mlp_uses_native_gemm():
    from p2pfl_amd.models.vit import Mlp

    torch.manual_seed(0)
    m = Mlp(768, 3072).cuda()
    x = torch.randn(2, 197, 768, device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = m(x)
    ref = m.fc2(F.gelu(m.fc1(x)))
    torch.testing.assert_close(y.float(), ref, atol=5e-2, rtol=5e-2)


# ---- 256 x 256 tile (TILE256: 8 waves, 128 x 64 per wave) -------------------------
@pytest.mark.parametrize("variant", [TILE256, TILE256 | A_PANEL])
@pytest.mark.parametrize("a_kmajor,b_kmajor", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (600, 520, 200), (1000, 768, 768), (72, 1000, 96)])
def test_gemm256_layouts_vs_fp32(monkeypatch, variant, a_kmajor, b_kmajor, M, N, K):
    """Every operand layout on the wide tile; ragged M / N / K and a grid smaller than one tile."""
    monkeypatch.setattr(gemm_mod, "_VARIANT_ENV", str(variant))
    a, b = _operands(M, N, K, a_kmajor, b_kmajor, seed=M + N + K + variant)
    out, _ = ops.gemm(a, b, a_kmajor, b_kmajor, out_dtype=torch.float32)
    ref, _ = ops.gemm_reference(a, b, a_kmajor, b_kmajor)
    torch.testing.assert_close(out, ref, atol=2e-3, rtol=1e-4)


def test_gemm256_exact_integers(monkeypatch):
    monkeypatch.setattr(gemm_mod, "_VARIANT_ENV", str(TILE256))
    M, N, K = 520, 392, 256
    A = torch.randint(-3, 4, (M, K), device="cuda").to(torch.bfloat16)
    B = (torch.arange(N * K, device="cuda").view(N, K) % 7 - 3).to(torch.bfloat16)
    for ak, bk in [(True, True), (True, False), (False, True), (False, False)]:
        a = A if ak else A.t().contiguous()
        b = B if bk else B.t().contiguous()
        out, _ = ops.gemm(a, b, ak, bk, out_dtype=torch.float32)
        assert torch.equal(out, A.float() @ B.float().t()), (ak, bk)
        outb, _ = ops.gemm(a, b, ak, bk, out_dtype=torch.bfloat16)  # LDS-staged bf16 epilogue
        assert torch.equal(outb, (A.float() @ B.float().t()).to(torch.bfloat16)), (ak, bk)


@pytest.mark.parametrize("splits", [2, 4, 8])
def test_gemm256_split_k(monkeypatch, splits):
    monkeypatch.setattr(gemm_mod, "_VARIANT_ENV", str(TILE256 | A_PANEL))
    M, N, K = 512, 768, 6304
    a, b = _operands(M, N, K, False, False, seed=splits)
    out, _ = ops.gemm(a, b, False, False, out_dtype=torch.bfloat16, splits=splits)
    ref, _ = ops.gemm_reference(a, b, False, False)
    torch.testing.assert_close(out.float(), ref, atol=0.5, rtol=1e-2)


def test_gemm256_epilogue_bias_gelu_residual(monkeypatch):
    monkeypatch.setattr(gemm_mod, "_VARIANT_ENV", str(TILE256))
    M, N, K = 700, 512, 192
    a, b = _operands(M, N, K, True, True, seed=5)
    bias = torch.randn(N, device="cuda")
    res = torch.randn(M, N, device="cuda").to(torch.bfloat16)
    out, z = ops.gemm(a, b, bias=bias, gelu=True, want_z=True, residual=res, out_dtype=torch.float32)
    ref, zref = ops.gemm_reference(a, b, bias=bias, gelu=True, residual=res)
    torch.testing.assert_close(out, ref, atol=2e-3, rtol=1e-4)
    torch.testing.assert_close(z.float(), zref, atol=3e-2, rtol=8e-3)
    outb, _ = ops.gemm(a, b, bias=bias, gelu=True, residual=res, out_dtype=torch.bfloat16)
    torch.testing.assert_close(outb.float(), ref, atol=5e-2, rtol=1e-2)


@pytest.mark.parametrize("m16", [False, True], ids=["mfma32", "mfma16"])
@pytest.mark.parametrize("a_kmajor,b_kmajor", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K", [(512, 512, 256), (296, 264, 128), (1000, 776, 448), (264, 520, 200)])
def test_pingpong_gemm_layouts_vs_fp32(a_kmajor, b_kmajor, M, N, K, m16):
    """The ping-pong 256 x 256 kernel (variant bit 11) in both MFMA forms (32x32x16, and
    16x16x32 with bit 16): every layout, M / N tails (clamped rows), odd K-tile counts,
    and (m/n-major only) a K tail through the buffer range check."""
    from p2pfl_amd.ops.gemm import PP, PP_M16, pp_eligible_any

    # a k-major K tail is not range-checked by this kernel: the planner never offers it
    # there, and a direct request runs on the 128 x 128 core kernel (checked below too)
    assert pp_eligible_any(M, N, K, a_kmajor, b_kmajor) == (not ((a_kmajor or b_kmajor) and K % 64))
    a, b = _operands(M, N, K, a_kmajor, b_kmajor, seed=M + 3 * N + K)
    out = torch.empty(M, N, device="cuda", dtype=torch.float32)
    ops.ext().gemm(a, b, a_kmajor, b_kmajor, out, None, False, None, None, 1, PP | (PP_M16 if m16 else 0))
    ref, _ = ops.gemm_reference(a, b, a_kmajor, b_kmajor)
    torch.testing.assert_close(out, ref, atol=2e-3, rtol=1e-4)


@pytest.mark.parametrize("m16", [False, True], ids=["mfma32", "mfma16"])
def test_pingpong_gemm_epilogues_and_split_k(m16):
    """Bias + GELU (+ pre-activation) and residual epilogues, bf16 out; split-K reduced in the launch."""
    from p2pfl_amd.ops.gemm import PP as PP0, PP_M16
    from p2pfl_amd.ops.splitk import counters, tiles_of

    PP = PP0 | (PP_M16 if m16 else 0)

    C = ops.ext()
    M, N, K = 6304, 3072, 768  # ViT-B/16 fc1: 300 tiles, the shape ops.gemm sends here
    a, b = _operands(M, N, K, True, True, seed=11)
    bias = torch.randn(N, device="cuda")
    out = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    z = torch.empty_like(out)
    C.gemm(a, b, True, True, out, bias, True, z, None, 1, PP)
    ref, zr = ops.gemm_reference(a, b, True, True, bias, True)
    torch.testing.assert_close(z.float(), zr, atol=0.25, rtol=1e-2)
    torch.testing.assert_close(out.float(), ref, atol=0.25, rtol=1e-2)
    res = torch.randn(M, 768, device="cuda").to(torch.bfloat16)
    a2, b2 = _operands(M, 768, 768, True, True, seed=12)
    out2 = torch.empty(M, 768, device="cuda", dtype=torch.bfloat16)
    C.gemm(a2, b2, True, True, out2, bias[:768].contiguous(), False, None, res, 1, PP)
    ref2, _ = ops.gemm_reference(a2, b2, True, True, bias[:768], False, res)
    torch.testing.assert_close(out2.float(), ref2, atol=0.25, rtol=1e-2)
    # weight-gradient shape: both operands m/n-major, K = 6304 tokens (tail), 3 slices
    a3, b3 = _operands(768, 768, 6304, False, False, seed=13)
    out3 = torch.empty(768, 768, device="cuda", dtype=torch.float32)
    ws = torch.empty(3 * 768 * 768, device="cuda")
    C.gemm(a3, b3, False, False, out3, None, False, None, None, 3, PP, ws, counters(tiles_of(768, 768), out3.device))
    ref3, _ = ops.gemm_reference(a3, b3, False, False)
    torch.testing.assert_close(out3, ref3, atol=5e-3, rtol=1e-4)


@pytest.mark.parametrize("kernel", ["128", "pingpong", "pingpong16"])
@pytest.mark.parametrize("splits", [2, 3, 4])
def test_in_launch_splitk_reused_workspace(splits, kernel):
    """Back-to-back in-launch split-K launches over ONE reused workspace and counter
    array, on a grid of many tiles (slices of a tile land on different XCDs): each
    launch must see only its own slabs (pins the sc1 hand-off assumption documented
    in csrc/gemm_core.h).  Integer operands make every summation order exact, so the
    in-launch reduction must equal the fp32 product bit for bit, launch after launch."""
    from p2pfl_amd.ops.splitk import counters, slab_elems, tiles_of

    from p2pfl_amd.ops.gemm import PP, PP_M16

    v = {"128": 0, "pingpong": PP, "pingpong16": PP | PP_M16}[kernel]
    C = ops.ext()
    M, N, K = 1024, 768, 2048  # 48 tiles (12 of 256 x 256) x splits workgroups
    ws = torch.empty(splits * slab_elems(M, N, v), device="cuda")
    cnt = counters(tiles_of(M, N), torch.device("cuda"))
    outs, refs = [], []
    for it in range(24):
        g = torch.Generator(device="cuda").manual_seed(100 + it)
        A = torch.randint(-2, 3, (M, K), device="cuda", generator=g).to(torch.bfloat16)
        B = torch.randint(-2, 3, (N, K), device="cuda", generator=g).to(torch.bfloat16)
        out = torch.empty(M, N, device="cuda", dtype=torch.float32)
        C.gemm(A.t().contiguous(), B.t().contiguous(), False, False, out, None, False, None, None, splits, v, ws, cnt)
        outs.append(out)
        refs.append(A.float() @ B.float().t())
    torch.cuda.synchronize()
    for it, (o, r) in enumerate(zip(outs, refs)):
        assert torch.equal(o, r), f"launch {it}: max err {(o - r).abs().max().item()}"
    if v:
        return
    # the separate-launch reducer on the same last operands agrees too
    ws2 = torch.empty(splits * slab_elems(M, N), device="cuda")
    out2 = torch.empty(M, N, device="cuda", dtype=torch.float32)
    C.gemm(A.t().contiguous(), B.t().contiguous(), False, False, ws2, None, False, None, None, splits, 0, None, None)
    C.tile_slab_reduce(ws2, splits, M, N, out2, 0)
    assert torch.equal(out2, refs[-1])


# ---- stream-K schedule of the ping-pong kernel (variant bits 11 + 17) ---------------------
@pytest.mark.parametrize("m16", [False, True], ids=["mfma32", "mfma16"])
@pytest.mark.parametrize("a_kmajor,b_kmajor", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K,grid", [(1000, 776, 448, 37), (512, 512, 1024, 24), (600, 264, 3072, 256),
                                        (264, 520, 200, 5), (6304 // 4, 768, 3072, 256), (256, 256, 64, 1)])
def test_stream_k_layouts_vs_fp32(a_kmajor, b_kmajor, M, N, K, grid, m16):
    """Stream-K: workgroups whose K-tile ranges cut tiles anywhere (grids that do and do
    not divide the iteration count, one workgroup spanning several tiles, several
    workgroups per tile), every operand layout, M / N tails, a K tail (m/n-major)."""
    from p2pfl_amd.ops.gemm import PP, PP_M16, PP_SK, sk_iters

    assert grid <= sk_iters(M, N, K)
    if (a_kmajor or b_kmajor) and K % 64:  # no fallback for the stream-K schedule: refused loudly
        a, b = _operands(M, N, K, a_kmajor, b_kmajor, seed=2)
        ws = torch.empty(2 * grid * gemm_mod.SK_SLAB, device="cuda")
        cnt = torch.zeros(-(-M // 128) * -(-N // 128), dtype=torch.int32, device="cuda")
        with pytest.raises(RuntimeError, match="stream-K"):
            ops.ext().gemm(a, b, a_kmajor, b_kmajor, torch.empty(M, N, device="cuda"), None, False, None, None, grid,
                           PP | PP_SK, ws, cnt)
        return
    a, b = _operands(M, N, K, a_kmajor, b_kmajor, seed=M + 5 * N + K)
    out, _ = ops.gemm(a, b, a_kmajor, b_kmajor, out_dtype=torch.float32, splits=grid,
                      variant=PP | PP_SK | (PP_M16 if m16 else 0))
    ref, _ = ops.gemm_reference(a, b, a_kmajor, b_kmajor)
    torch.testing.assert_close(out, ref, atol=5e-3, rtol=1e-4)


@pytest.mark.parametrize("m16", [False, True], ids=["mfma32", "mfma16"])
def test_stream_k_epilogues(m16):
    """Bias + GELU (+ pre-activation) and bias + residual epilogues applied by the
    workgroup that completes each cut tile, bf16 out (the ViT fc1 / proj shapes)."""
    from p2pfl_amd.ops.gemm import PP, PP_M16, PP_SK

    v = PP | PP_SK | (PP_M16 if m16 else 0)
    M, N, K = 6304, 3072, 768
    a, b = _operands(M, N, K, True, True, seed=21)
    bias = torch.randn(N, device="cuda")
    out, z = ops.gemm(a, b, bias=bias, gelu=True, want_z=True, splits=256, variant=v)
    ref, zr = ops.gemm_reference(a, b, True, True, bias, True)
    torch.testing.assert_close(z.float(), zr, atol=0.25, rtol=1e-2)
    torch.testing.assert_close(out.float(), ref, atol=0.25, rtol=1e-2)
    res = torch.randn(M, 768, device="cuda").to(torch.bfloat16)
    a2, b2 = _operands(M, 768, 3072, True, True, seed=22)
    out2, _ = ops.gemm(a2, b2, bias=bias[:768].to(torch.bfloat16), residual=res, splits=200, variant=v)
    ref2, _ = ops.gemm_reference(a2, b2, True, True, bias[:768].to(torch.bfloat16), False, res)
    torch.testing.assert_close(out2.float(), ref2, atol=0.5, rtol=1e-2)


@pytest.mark.parametrize("grid", [96, 256])
def test_stream_k_reused_workspace_bitwise(grid):
    """Back-to-back stream-K launches over one reused counter array: every launch sees
    only its own partials (the sc1 hand-off), and the fix-up sums the partials in a
    fixed order whichever workgroup completes a tile, so repeated launches on the same
    operands are bitwise identical (random operands: summation order matters)."""
    from p2pfl_amd.ops.gemm import PP, PP_SK, SK_SLAB
    from p2pfl_amd.ops.splitk import counters, tiles_of

    C = ops.ext()
    V = PP | PP_SK
    M, N, K = 6304, 768, 3072  # the fc2 forward: 75 tiles of 48 K-tiles
    cnt = counters(tiles_of(M, N), torch.device("cuda"))
    ws = torch.empty(2 * grid * SK_SLAB, device="cuda")
    a, b = _operands(M, N, K, True, True, seed=31)
    outs = []
    for it in range(12):
        out = torch.empty(M, N, device="cuda", dtype=torch.float32)
        C.gemm(a, b, True, True, out, None, False, None, None, grid, V, ws, cnt)
        outs.append(out)
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0, "tile counters must be left zero"
    ref, _ = ops.gemm_reference(a, b)
    torch.testing.assert_close(outs[0], ref, atol=5e-3, rtol=1e-4)
    for it, o in enumerate(outs[1:], 1):
        assert torch.equal(o, outs[0]), f"launch {it} differs: max {(o - outs[0]).abs().max().item()}"
    # integer operands: exact whatever the order, across a fresh operand every launch
    for it in range(8):
        g = torch.Generator(device="cuda").manual_seed(200 + it)
        A = torch.randint(-2, 3, (M, K), device="cuda", generator=g).to(torch.bfloat16)
        B = torch.randint(-2, 3, (N, K), device="cuda", generator=g).to(torch.bfloat16)
        out = torch.empty(M, N, device="cuda", dtype=torch.float32)
        C.gemm(A, B, True, True, out, None, False, None, None, grid, V, ws, cnt)
        assert torch.equal(out, A.float() @ B.float().t()), it


def test_stream_k_refuses_bad_grid():
    from p2pfl_amd.ops.gemm import PP, PP_SK, sk_iters

    a, b = _operands(256, 256, 128, True, True)
    with pytest.raises(RuntimeError):
        ops.gemm(a, b, splits=sk_iters(256, 256, 128) + 1, variant=PP | PP_SK)


# ---- 256 x 128 ping-pong tile (PP | PP_N128) --------------------------------------
@pytest.mark.parametrize("m16", [False, True], ids=["mfma32", "mfma16"])
@pytest.mark.parametrize("a_kmajor,b_kmajor", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("M,N,K", [(512, 256, 256), (296, 200, 128), (1000, 776, 448), (264, 520, 200), (6304, 768, 3072),
                                   (72, 136, 64)])
def test_pingpong128_layouts_vs_fp32(a_kmajor, b_kmajor, M, N, K, m16):
    """The 256 x 128 tile: every layout, M / N tails (clamped rows, masked stores), odd and
    even K-tile counts (the two-K-tile phase schedule's tail), a K tail (m/n-major only)."""
    from p2pfl_amd.ops.gemm import PP, PP_M16, PP_N128, pp_eligible_any

    # k-major K tail: never planned on this kernel; a direct request runs on the core kernel
    assert pp_eligible_any(M, N, K, a_kmajor, b_kmajor) == (not ((a_kmajor or b_kmajor) and K % 64))
    v = PP | PP_N128 | (PP_M16 if m16 else 0)
    a, b = _operands(M, N, K, a_kmajor, b_kmajor, seed=M + 7 * N + K)
    out, _ = ops.gemm(a, b, a_kmajor, b_kmajor, out_dtype=torch.float32, variant=v)
    ref, _ = ops.gemm_reference(a, b, a_kmajor, b_kmajor)
    torch.testing.assert_close(out, ref, atol=5e-3, rtol=1e-4)
    outb, _ = ops.gemm(a, b, a_kmajor, b_kmajor, out_dtype=torch.bfloat16, variant=v)
    torch.testing.assert_close(outb.float(), ref, atol=0.25, rtol=1e-2)


@pytest.mark.parametrize("m16", [False, True], ids=["mfma32", "mfma16"])
def test_pingpong128_exact_integers_and_epilogues(m16):
    from p2pfl_amd.ops.gemm import PP, PP_M16, PP_N128

    v = PP | PP_N128 | (PP_M16 if m16 else 0)
    M, N, K = 520, 392, 256
    A = torch.randint(-3, 4, (M, K), device="cuda").to(torch.bfloat16)
    B = (torch.arange(N * K, device="cuda").view(N, K) % 7 - 3).to(torch.bfloat16)
    for ak, bk in [(True, True), (True, False), (False, True), (False, False)]:
        a = A if ak else A.t().contiguous()
        b = B if bk else B.t().contiguous()
        out, _ = ops.gemm(a, b, ak, bk, out_dtype=torch.float32, variant=v)
        assert torch.equal(out, A.float() @ B.float().t()), (ak, bk)
    # bias + GELU (+ pre-activation), bias + residual (the ViT fc2 / proj forward)
    M, N, K = 6304, 768, 3072
    a, b = _operands(M, N, K, True, True, seed=41)
    bias = torch.randn(N, device="cuda")
    out, z = ops.gemm(a, b, bias=bias, gelu=True, want_z=True, variant=v)
    ref, zr = ops.gemm_reference(a, b, True, True, bias, True)
    torch.testing.assert_close(z.float(), zr, atol=0.5, rtol=1e-2)
    torch.testing.assert_close(out.float(), ref, atol=0.5, rtol=1e-2)
    res = torch.randn(M, N, device="cuda").to(torch.bfloat16)
    out2, _ = ops.gemm(a, b, bias=bias.to(torch.bfloat16), residual=res, variant=v)
    ref2, _ = ops.gemm_reference(a, b, True, True, bias.to(torch.bfloat16), False, res)
    torch.testing.assert_close(out2.float(), ref2, atol=0.5, rtol=1e-2)
    with pytest.raises(RuntimeError):
        ops.gemm(a, b, splits=2, variant=v)


@pytest.mark.parametrize("m16", [False, True], ids=["mfma32", "mfma16"])
@pytest.mark.parametrize("kind", ["fwd_gelu", "dgrad", "wgrad_layout"])
def test_rowsplit_vs_fp32(kind, m16):
    """Row-split schedule (variant bit 22): one full wave of 256 x 256 tiles over the first
    rows, the 256 x 128 tile over the rest, as two launches on row views of A / C / z."""
    from p2pfl_amd.ops.gemm import PP, PP_M16, PP_ROWSPLIT, rowsplit_rows

    v = PP | PP_ROWSPLIT | (PP_M16 if m16 else 0)
    M, N, K = 6304, 3072, 768
    assert rowsplit_rows(M, N) == 5376
    if kind == "fwd_gelu":
        a, b = _operands(M, N, K, True, True, seed=51)
        bias = torch.randn(N, device="cuda")
        out, z = ops.gemm(a, b, bias=bias, gelu=True, want_z=True, variant=v)
        ref, zr = ops.gemm_reference(a, b, True, True, bias, True)
        torch.testing.assert_close(z.float(), zr, atol=0.25, rtol=1e-2)
        torch.testing.assert_close(out.float(), ref, atol=0.25, rtol=1e-2)
    elif kind == "dgrad":
        a, b = _operands(M, N, K, True, False, seed=52)
        out, _ = ops.gemm(a, b, True, False, out_dtype=torch.float32, variant=v)
        ref, _ = ops.gemm_reference(a, b, True, False)
        torch.testing.assert_close(out, ref, atol=5e-3, rtol=1e-4)
    else:  # m-major A: the row split is a column view of the stored operand
        a, b = _operands(M, N, K, False, True, seed=53)
        out, _ = ops.gemm(a, b, False, True, out_dtype=torch.float32, variant=v)
        ref, _ = ops.gemm_reference(a, b, False, True)
        torch.testing.assert_close(out, ref, atol=5e-3, rtol=1e-4)


@pytest.mark.parametrize("v_name", ["pingpong", "ring"])
@pytest.mark.parametrize("splits", [6, 8])
def test_forced_in_launch_split_k_beyond_four_slices(v_name, splits):
    """GEMM_IL: the weight-gradient configurations that reduce 6-8 K-slices in the launch
    (instead of slabs + a separate reduce) equal the fp32 product exactly on integer
    operands (m-major operands, the wgrad layout)."""
    import importlib

    g_mod = importlib.import_module("p2pfl_amd.ops.gemm")
    v = {"pingpong": g_mod.PP, "ring": g_mod.RING4 | g_mod.A_PANEL}[v_name] | g_mod.GEMM_IL
    M, N, K = 768, 3072, 6304  # dW = dY^T X of the ViT-B fc products, K = tokens
    g = torch.Generator(device="cuda").manual_seed(splits)
    dy = torch.randint(-2, 3, (K, M), device="cuda", generator=g).to(torch.bfloat16)
    x = torch.randint(-2, 3, (K, N), device="cuda", generator=g).to(torch.bfloat16)
    assert g_mod._cfg_ok(v, splits, M, N, K, False, False, False)
    for _ in range(3):
        out, _ = g_mod.gemm(dy, x, False, False, out_dtype=torch.float32, splits=splits, variant=v)
        torch.testing.assert_close(out, dy.float().t() @ x.float(), atol=0, rtol=0)


@pytest.mark.parametrize("m16", [False, True], ids=["mfma32", "mfma16"])
def test_pingpong_exact_integers(m16):
    """The 256 x 256 ping-pong tile, unsplit, on small integers (every partial sum at most
    1728 in magnitude: exact in fp32): 3 x 2 tiles with M and N tails and three K-tiles (the
    odd-count exit of the two-tile loop), every layout; the bf16 output pins the LDS
    staging store (both sides round to nearest even)."""
    from p2pfl_amd.ops.gemm import PP, PP_M16

    v = PP | (PP_M16 if m16 else 0)
    M, N, K = 520, 392, 192
    A = torch.randint(-3, 4, (M, K), device="cuda").to(torch.bfloat16)
    B = (torch.arange(N * K, device="cuda").view(N, K) % 7 - 3).to(torch.bfloat16)
    ref = A.float() @ B.float().t()
    for ak, bk in [(True, True), (True, False), (False, True), (False, False)]:
        a = A if ak else A.t().contiguous()
        b = B if bk else B.t().contiguous()
        out, _ = ops.gemm(a, b, ak, bk, out_dtype=torch.float32, variant=v)
        assert torch.equal(out, ref), (ak, bk)
        outb, _ = ops.gemm(a, b, ak, bk, out_dtype=torch.bfloat16, variant=v)
        assert torch.equal(outb, ref.to(torch.bfloat16)), (ak, bk)


def test_pingpong_refuses_unassigned_bits():
    """Bits 12-15 and 18-20 select nothing with the ping-pong bit: a forced or stale value
    fails in the binding (it neither runs nor falls through to the core kernels, where
    bit 12 is the ring and bit 14 the convolutions' 64 x 64 tile)."""
    from p2pfl_amd.ops.gemm import PP, PP_SK, SK_SLAB
    from p2pfl_amd.ops.splitk import counters, tiles_of

    M, N, K = 256, 256, 64
    a, b = _operands(M, N, K, True, True)
    out = torch.empty(M, N, device="cuda")
    with pytest.raises(RuntimeError):
        ops.ext().gemm(a, b, True, True, out, None, False, None, None, 1, PP | (1 << 14))
    ws = torch.empty(2 * SK_SLAB, device="cuda")
    cnt = counters(tiles_of(M, N), torch.device("cuda"))
    with pytest.raises(RuntimeError):
        ops.ext().gemm(a, b, True, True, out, None, False, None, None, 1, PP | PP_SK | (1 << 20), ws, cnt)


def test_variant_names_match_extension():
    """csrc/gemm.h's constants, as the extension exports them, equal ops/variant.py's."""
    from p2pfl_amd.ops import variant

    names = {k: v for k, v in vars(variant).items() if k.isupper() and isinstance(v, int)}
    assert dict(ops.ext().gemm_variant_bits) == names
    assert (gemm_mod.PP, gemm_mod.PP_M16, gemm_mod.PP_SK, gemm_mod.PP_N128) == (2048, 1 << 16, 1 << 17, 1 << 21)
