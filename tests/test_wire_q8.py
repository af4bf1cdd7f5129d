"""The block-quantised int8 model wire (``Settings.WIRE_DTYPE = "q8"``) on the CPU:
the reference codec, the raw-block rule, the frame and two-node rounds."""

from __future__ import annotations

import json
import math
import struct
import time

import pytest
import torch

from p2pfl_amd import ops
from p2pfl_amd.learning import wire
from p2pfl_amd.learning.arena import FlatParams, flatten, q8_raw_blocks
from p2pfl_amd.learning.exceptions import DecodingParamsError
from p2pfl_amd.learning.wire import decode_params, encode_params
from p2pfl_amd.models import CNN, MLP
from p2pfl_amd.settings import Settings

FLT_MIN = 2.0**-126
SIZES = [1, 63, 64, 65, 4099]
TIE_BLOCK = [127.0, 0.5, 1.5, 2.5, -0.5, -1.5, 126.5, -126.5]
TIE_CODES = [127, 0, 2, 2, 0, -2, 126, -126]


@pytest.fixture
def q8_wire():
    old = Settings.WIRE_DTYPE
    Settings.WIRE_DTYPE = "q8"
    yield
    Settings.WIRE_DTYPE = old


def sections(packed: torch.Tensor, n: int, n_raw: int = 0):
    """(int8 codes [nb, 64], fp32 raw [R, 64], fp32 scales [nb]) of a packed buffer."""
    nb = -(-n // 64)
    c, r = 64 * nb, 256 * n_raw
    assert packed.dtype == torch.uint8 and packed.numel() == c + r + 4 * nb
    p = packed.cpu()
    return (p[:c].clone().view(torch.int8).view(nb, 64), p[c : c + r].clone().view(torch.float32).view(n_raw, 64),
            p[c + r :].clone().view(torch.float32))


def scaled_gaussian(n: int, sigma: float, seed: int) -> torch.Tensor:
    """Gaussians with a log-normal magnitude per 64-element block."""
    g = torch.Generator().manual_seed(seed)
    nb = -(-n // 64)
    mag = torch.exp(sigma * torch.randn(nb, 1, generator=g))
    return (torch.randn(nb, 64, generator=g) * mag).reshape(-1)[:n].contiguous()


def assert_error_bound(x: torch.Tensor, y: torch.Tensor, packed: torch.Tensor, raw=()):
    """|y - x| <= 0.5 scale + 2^-22 amax for every non-raw element of a block
    with a finite, non-zero scale; a zero-scale block holds only |x| < 127 FLT_MIN."""
    n = x.numel()
    nb = -(-n // 64)
    _, _, scales = sections(packed, n, len(raw))
    pad = torch.zeros(nb * 64, dtype=torch.float64)
    out = pad.clone()
    pad[:n] = x.double().cpu()
    out[:n] = y.double().cpu()
    xb, yb, s = pad.view(nb, 64), out.view(nb, 64), scales.double()
    err = (yb - xb).abs()
    amax = xb.abs().max(dim=1).values
    keep = torch.ones(nb, dtype=torch.bool)
    keep[list(raw)] = False
    finite = torch.isfinite(s) & keep
    assert bool(finite.any())
    bound = 0.5 * s + 2.0**-22 * amax
    live = finite & (s > 0)
    assert bool((err[live] <= bound[live][:, None]).all()), float((err[live] / bound[live][:, None]).max())
    zero = finite & (s == 0)
    assert bool((amax[zero] < 127 * FLT_MIN).all()) and not bool(yb[zero].any())
    return float((err[live] / (0.5 * s[live][:, None])).max()) if bool(live.any()) else 0.0


# ---------------------------------------------------------------------------
# reference properties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("sigma", [0.0, 3.0, 12.0])
def test_reference_error_bound_and_code_range(n, sigma):
    x = scaled_gaussian(n, sigma, seed=n)
    packed = ops.q8_encode_reference(x)
    codes, _, scales = sections(packed, n)
    assert int(codes.abs().max()) <= 127 and int(codes.min()) >= -127
    assert bool((codes.reshape(-1)[n:] == 0).all())  # tail padding
    amax = torch.zeros(codes.shape[0] * 64)
    amax[:n] = x.abs()
    assert torch.equal(scales, amax.view(-1, 64).max(dim=1).values / 127.0)
    y = ops.q8_decode_reference(packed, n)
    assert y.dtype == torch.float32 and y.shape == (n,)
    assert assert_error_bound(x, y, packed) <= 1.0 + 2.0**-20


def test_reference_ties_to_even():
    x = torch.zeros(64)
    x[:8] = torch.tensor(TIE_BLOCK)
    codes, _, scales = sections(ops.q8_encode_reference(x), 64)
    assert scales.tolist() == [1.0]
    assert codes[0, :8].tolist() == TIE_CODES
    assert not bool(codes[0, 8:].any())


def test_reference_keeps_subnormal_elements_of_a_quantised_block():
    """The zero-scale rule makes a block of subnormals independent of denormal
    flushing; a subnormal element of a block that is quantised is not: the
    format is IEEE binary32 with subnormals kept (0.75 FLT_MIN / FLT_MIN rounds to 1)."""
    x = torch.zeros(64)
    x[0], x[1], x[2] = 127 * FLT_MIN, 0.75 * FLT_MIN, -0.75 * FLT_MIN
    codes, _, scales = sections(ops.q8_encode_reference(x), 64)
    assert scales[0] == FLT_MIN and codes[0, :3].tolist() == [127, 1, -1]


def test_reference_zero_and_subnormal_blocks_have_zero_scale():
    x = torch.ones(192)
    x[:64] = 0.0
    x[64:128] = torch.linspace(-1.0, 1.0, 64) * 2.0**-127  # subnormals
    x[127] = 126.99 * FLT_MIN  # just below the threshold, a normal number
    packed = ops.q8_encode_reference(x)
    codes, _, scales = sections(packed, 192)
    assert scales.view(torch.int32).tolist()[:2] == [0, 0] and scales[2] == 1.0 / 127.0
    assert not bool(codes[:2].any())
    y = ops.q8_decode_reference(packed, 192)
    assert not bool(y[:128].any()) and torch.equal(y[128:], (torch.tensor(127.0) * scales[2]).expand(64))
    # at the threshold the block is quantised
    x[127] = 127 * FLT_MIN
    _, _, scales = sections(ops.q8_encode_reference(x), 192)
    assert scales[1] == FLT_MIN


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_reference_non_finite_poisons_exactly_its_block(bad):
    x = scaled_gaussian(320, 1.0, seed=3)
    x[130] = bad  # block 2
    packed = ops.q8_encode_reference(x)
    codes, _, scales = sections(packed, 320)
    assert scales.view(torch.int32)[2] == 0x7FC00000 and not bool(codes[2].any())
    y = ops.q8_decode_reference(packed, 320).view(5, 64)
    assert bool(torch.isnan(y[2]).all())
    others = [0, 1, 3, 4]
    assert bool(torch.isfinite(y[others]).all()) and bool(torch.isfinite(scales[others]).all())
    clean = x.clone()
    clean[130] = 0.0
    assert torch.equal(y[others], ops.q8_decode_reference(ops.q8_encode_reference(clean), 320).view(5, 64)[others])


@pytest.mark.parametrize("n", SIZES)
def test_reference_raw_blocks_come_back_bit_exact(n):
    x = scaled_gaussian(n, 3.0, seed=7 * n)
    nb = -(-n // 64)
    raw = sorted({0, nb // 2, nb - 1})
    packed = ops.q8_encode_reference(x, raw)
    assert packed.numel() == ops.q8_packed_nbytes(n, len(raw))
    # raw blocks are still encoded as ordinary blocks in the codes and scales sections
    plain = ops.q8_encode_reference(x)
    codes, rawsec, scales = sections(packed, n, len(raw))
    pcodes, _, pscales = sections(plain, n)
    assert torch.equal(codes, pcodes) and torch.equal(scales.view(torch.int32), pscales.view(torch.int32))
    pad = torch.zeros(nb * 64)
    pad[:n] = x
    assert torch.equal(rawsec, pad.view(nb, 64)[raw])
    y = ops.q8_decode_reference(packed, n, raw)
    mask = torch.zeros(nb * 64, dtype=torch.bool)
    for b in raw:
        mask[b * 64 : (b + 1) * 64] = True
    mask = mask[:n]
    assert torch.equal(y[mask].view(torch.int32), x[mask].view(torch.int32))
    assert torch.equal(y[~mask], ops.q8_decode_reference(plain, n)[~mask])
    if len(raw) < nb:
        assert_error_bound(x, y, packed, raw)
    yb = ops.q8_decode_reference(packed, n, raw, out_dtype=torch.bfloat16)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb, y.to(torch.bfloat16))


@pytest.mark.parametrize("n", SIZES)
def test_reference_bf16_input_equals_its_widened_fp32(n):
    x = scaled_gaussian(n, 3.0, seed=n + 1).to(torch.bfloat16)
    assert torch.equal(ops.q8_encode_reference(x, [0]), ops.q8_encode_reference(x.float(), [0]))
    assert torch.equal(ops.q8_encode(x, [0]), ops.q8_encode_reference(x.float(), [0]))  # the op serves CPU tensors


def test_packed_nbytes_matches_the_section_table():
    assert ops.Q8_BLOCK == 64
    for n, r in [(1, 0), (63, 1), (64, 0), (65, 2), (4099, 5), (6_497_280, 35)]:
        nb = math.ceil(n / 64)
        assert ops.q8_packed_nbytes(n, r) == 64 * nb + 256 * r + 4 * nb
        assert (64 * nb) % 64 == 0 and (64 * nb + 256 * r) % 64 == 0  # sections start 64-byte aligned
    assert ops.q8_packed_nbytes(64) == 68
    with pytest.raises(ValueError):
        ops.q8_packed_nbytes(0)
    with pytest.raises(ValueError):
        ops.q8_decode_reference(torch.zeros(67, dtype=torch.uint8), 64)
    for bad in ([1, 0], [0, 0], [2], [-1]):
        with pytest.raises(ValueError):
            ops.q8_encode_reference(torch.ones(128), bad)


# ---------------------------------------------------------------------------
# which blocks are raw
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("model,count", [(MLP, 7), (CNN, 35)])
def test_raw_blocks_are_the_blocks_of_tensors_with_at_most_one_dimension(model, count):
    layout = flatten(model().state_dict()).layout
    blocks = q8_raw_blocks(layout)
    expect = []
    for shape, off, size in zip(layout.shapes, layout.offsets, layout.sizes()):
        if len(shape) <= 1:
            expect += [b for b in range(layout.numel // 64) if off <= b * 64 < off + size]
    assert list(blocks) == expect and len(blocks) == count
    assert list(blocks) == sorted(set(blocks)) and blocks[-1] < layout.numel // 64
    assert q8_raw_blocks(layout) is blocks  # cached beside the layout
    ratio = ops.q8_packed_nbytes(layout.numel, count) / (4 * layout.numel)
    assert 0.265 < ratio < 0.268


# ---------------------------------------------------------------------------
# frame
# ---------------------------------------------------------------------------
def _reframe(frame: bytes, header=None, body=None) -> bytes:
    """The frame with another header and / or body and a matching CRC."""
    _v, hbytes, old_body = wire._validate(memoryview(frame))
    return wire._pack(json.loads(hbytes.decode()) if header is None else header, bytes(old_body) if body is None else body)


def _header(frame: bytes) -> dict:
    return json.loads(wire._validate(memoryview(frame))[1].decode())


def test_frame_round_trip_and_rejections(q8_wire):
    fp = flatten(MLP(seed=3).state_dict())
    raw = q8_raw_blocks(fp.layout)
    frame = encode_params(fp)
    hdr = _header(frame)
    assert (hdr["kind"], hdr["enc"], hdr["block"], hdr["raw"]) == ("flat", "q8", 64, len(raw))
    back = decode_params(frame)
    assert isinstance(back, FlatParams) and back.flat.dtype == torch.float32 and back.layout == fp.layout
    ref = ops.q8_decode_reference(ops.q8_encode_reference(fp.flat, raw), fp.layout.numel, raw)
    assert torch.equal(back.flat, ref)
    for name, t in fp.items():
        if t.dim() <= 1:
            assert torch.equal(back[name], t)
    Settings.WIRE_DTYPE = "fp32"
    fp32_frame = encode_params(fp)
    Settings.WIRE_DTYPE = "q8"
    assert len(frame) <= 0.28 * len(fp32_frame)
    # an fp32 frame still decodes with q8 set
    assert torch.equal(decode_params(fp32_frame).flat, fp.flat)

    body = bytes(wire._validate(memoryview(frame))[2])
    bad = {
        "truncated": _reframe(frame, body=body[:-1]),
        "extended": _reframe(frame, body=body + b"\0"),
        "block": _reframe(frame, header=dict(hdr, block=32)),
        "enc": _reframe(frame, header=dict(hdr, enc="q4")),
        "raw": _reframe(frame, header=dict(hdr, raw=len(raw) + 1)),
    }
    for what, data in bad.items():
        wire._validate(memoryview(data))  # the frame itself is sound: the q8 check must fire
        with pytest.raises(DecodingParamsError):
            decode_params(data)
    # the layout comes from the peer too: a frame whose layout is malformed, or implies another
    # size than the body has, is refused by arithmetic, before anything is built from its numbers
    lay = hdr["layout"]

    def with_layout(**kw):
        return _reframe(frame, header=dict(hdr, layout=dict(lay, **kw)))

    huge = [list(sh) for sh in lay["shapes"]]
    huge[-1] = [640_000_000_000]  # the last bias
    consistent = dict(lay, shapes=huge, numel=lay["offsets"][-1] + 640_000_000_000)  # well formed, only far too big
    hostile = {
        "huge shape": with_layout(shapes=huge),
        "huge and well formed": _reframe(frame, header=dict(hdr, layout=consistent, raw=len(raw) - 1 + 10_000_000_000)),
        "negative offset": with_layout(offsets=[-64] + lay["offsets"][1:]),
        "unaligned offset": with_layout(offsets=lay["offsets"][:-1] + [lay["offsets"][-1] + 1]),
        "overlapping tensors": with_layout(offsets=[lay["offsets"][0]] * len(lay["offsets"])),
        "negative dimension": with_layout(shapes=[[-1, -lay["shapes"][0][0] * lay["shapes"][0][1]]] + lay["shapes"][1:]),
        "missing entry": with_layout(offsets=lay["offsets"][:-1]),
        "numel 0": with_layout(numel=0),
    }
    from p2pfl_amd.learning import arena

    def no_expansion(layout):
        raise AssertionError("the raw-block list was expanded for a refused frame")

    expand, arena.q8_raw_blocks = arena.q8_raw_blocks, no_expansion
    try:
        for what, data in hostile.items():
            wire._validate(memoryview(data))
            with pytest.raises(DecodingParamsError):
                decode_params(data)
    finally:
        arena.q8_raw_blocks = expand
    assert all(layout.well_formed() and layout.numel < 10**9 for layout in arena._Q8_RAW)
    # a flipped body byte is still caught by the CRC
    flipped = bytearray(frame)
    flipped[-5] ^= 0x10
    with pytest.raises(DecodingParamsError, match="checksum"):
        decode_params(bytes(flipped))
    # the frame prefix is the unchanged version 2
    assert frame[:4] == b"P2FA" and struct.unpack("<I", frame[4:8])[0] == 2


def test_dict_payloads_and_reference_format_are_untouched(q8_wire):
    from collections import OrderedDict

    d = OrderedDict(w=torch.randn(70), b=torch.arange(5))
    out = decode_params(encode_params(d))
    assert torch.equal(out["w"], d["w"]) and torch.equal(out["b"], d["b"])
    fp = flatten(MLP(seed=1).state_dict())
    old = Settings.WIRE_FORMAT
    Settings.WIRE_FORMAT = "reference"
    try:
        got = decode_params(encode_params(fp))
    finally:
        Settings.WIRE_FORMAT = old
    assert isinstance(got, list) and all(torch.equal(torch.as_tensor(a), b) for a, b in zip(got, fp.values()))


# ---------------------------------------------------------------------------
# two nodes
# ---------------------------------------------------------------------------
def _q(flat, layout):
    raw = q8_raw_blocks(layout)
    return ops.q8_decode_reference(ops.q8_encode_reference(flat, raw), layout.numel, raw)


def test_two_members_exchanging_q8_frames_stay_within_the_quantisation_bound(q8_wire):
    """The exchange of one round written out: each member averages its own
    fp32 model with the decoded frame of the other's.  The aggregates differ by
    ((x0 - Q(x0)) - (x1 - Q(x1))) / 2, each term at most scale / 2 = amax / 254."""
    from p2pfl_amd.learning.aggregators.fedavg import FedAvg

    x = [flatten(MLP(seed=i).state_dict()) for i in range(2)]
    frames = [encode_params(p) for p in x]
    aggs = []
    for me in range(2):
        other = decode_params(frames[1 - me])
        aggs.append(FedAvg(f"n{me}").aggregate({f"n{me}": (x[me], 1), f"n{1 - me}": (other, 1)}).flat)
    amax = max(float(p.flat.abs().max()) for p in x)
    assert float((aggs[0] - aggs[1]).abs().max()) <= 1.01 * amax / 254
    mean = ((x[0].flat.double() + x[1].flat.double()) / 2).float()
    for a in aggs:
        assert float((a - mean).abs().max()) <= 1.01 * amax / 254


def run_two_nodes(protocol, model=MLP, **node_kw):
    """One round, epochs=0, of two nodes built from ``model(seed=i)``; returns
    (initial flats, final flats, layout, node addresses).

    The initiator's model reaches the other node as the ``init_model`` of the
    experiment, over the same wire: with epochs=0 both members enter the round
    with the initiator's model x0 (node 1 with its decoded copy), so the exact
    fp32 mean of the two members' models is x0 itself.
    """
    from p2pfl_amd.data import MnistFederatedDM
    from p2pfl_amd.node import Node
    from p2pfl_amd.utils import set_test_settings, wait_4_results, wait_convergence

    set_test_settings()
    models = [model(seed=i) for i in range(2)]
    init = [flatten(m.state_dict()) for m in models]
    init = [FlatParams.from_flat(p.flat.clone(), p.layout) for p in init]
    nodes = [Node(models[i], MnistFederatedDM(sub_id=i, number_sub=400), protocol=protocol, **node_kw) for i in range(2)]
    for nd in nodes:
        nd.start()
    try:
        nodes[1].connect(nodes[0].addr)
        wait_convergence(nodes, 1, only_direct=True, wait=10)
        nodes[0].set_start_learning(rounds=1, epochs=0)
        # the experiment starts on each node's own thread: wait_4_results only means
        # "finished" once every node has begun (the learner outlives the experiment)
        deadline = time.monotonic() + 60
        while any(nd.state.learner is None for nd in nodes):
            assert time.monotonic() < deadline, "learning did not start"
            time.sleep(0.01)
        wait_4_results(nodes, timeout=120)  # both nodes finish
        final = []
        for nd in nodes:
            from p2pfl_amd.learning.arena import reading

            params = nd.state.learner.get_parameters()
            with reading(params):
                final.append(params.flat[: params.layout.numel].detach().float().cpu().clone())
        return init, final, init[0].layout, [nd.addr for nd in nodes]
    finally:
        for nd in nodes:
            nd.stop()


def assert_round_within_quantisation_bound(init, final):
    amax = max(float(p.flat.abs().max()) for p in init)
    print(f"max |node0 - node1| = {float((final[0] - final[1]).abs().max()):.3e}, "
          f"max |node - x0| = {max(float((f - init[0].flat).abs().max()) for f in final):.3e}, "
          f"bound 1.01 amax / 254 = {1.01 * amax / 254:.3e}")
    assert float((final[0] - final[1]).abs().max()) <= 1.01 * amax / 254
    # every model that entered the round is the initiator's (see run_two_nodes): their exact fp32 mean is x0
    for f in final:
        assert float((f - init[0].flat).abs().max()) <= 1.01 * amax / 254
    # tensors of at most one dimension travel exactly
    layout = init[0].layout
    for b in q8_raw_blocks(layout):
        assert torch.equal(final[0][b * 64 : (b + 1) * 64], final[1][b * 64 : (b + 1) * 64])


def test_two_grpc_nodes(q8_wire):
    from p2pfl_amd.communication.grpc import GrpcCommunicationProtocol

    init, final, _, _ = run_two_nodes(GrpcCommunicationProtocol, device="cpu")
    assert_round_within_quantisation_bound(init, final)


def test_two_xgmi_sim_nodes_on_the_cpu(q8_wire):
    from p2pfl_amd.communication.xgmi import XgmiSimNetwork
    from p2pfl_amd.management.logger import logger

    init, final, layout, addrs = run_two_nodes(XgmiSimNetwork().protocol, device="cpu")
    assert_round_within_quantisation_bound(init, final)
    packed = ops.q8_packed_nbytes(layout.numel, len(q8_raw_blocks(layout)))
    pushes = 0
    for a in addrs:
        c = logger.tracer.counters(a)
        pushes += c.get("xgmi_pushes", 0)
        assert c.get("xgmi_bytes_sent", 0) == c.get("xgmi_pushes", 0) * packed
    assert pushes >= 2  # the init model and at least one model of the round crossed the plane
    recv = sum(logger.tracer.counters(a).get("xgmi_bytes_recv", 0) for a in addrs)
    assert recv >= 2 * packed and recv % packed == 0  # receivers count the packed bytes too


# ---------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------
def test_mnist_example_takes_wire_dtype(monkeypatch):
    from p2pfl_amd.examples import mnist

    assert mnist.parse_args([]).wire_dtype is None
    assert mnist.parse_args(["--wire_dtype", "q8", "--protocol", "grpc"]).wire_dtype == "q8"
    with pytest.raises(SystemExit):
        mnist.parse_args(["--wire_dtype", "q4"])
    seen = {}
    monkeypatch.setattr(mnist, "mnist", lambda *a, **k: seen.setdefault("wire", Settings.WIRE_DTYPE))
    monkeypatch.setattr(Settings, "WIRE_DTYPE", "fp32")
    monkeypatch.setattr(Settings, "LOG_LEVEL", Settings.LOG_LEVEL)
    mnist.main(["--wire_dtype", "q8"])
    assert seen["wire"] == "q8"
    # without the flag a setting the caller made stays
    Settings.WIRE_DTYPE = "bf16"
    seen.clear()
    mnist.main([])
    assert seen["wire"] == "bf16"


def test_layout_checks_and_bounded_caches():
    from p2pfl_amd.learning import arena
    from p2pfl_amd.learning.arena import ParamLayout, q8_raw_count

    for model in (MLP, CNN):
        layout = flatten(model().state_dict()).layout
        assert layout.well_formed() and q8_raw_count(layout) == len(q8_raw_blocks(layout))
    base = flatten(MLP().state_dict()).layout
    bad = ParamLayout(base.names, base.shapes, base.dtypes, (64,) + base.offsets[1:], base.numel)  # not in offset order
    assert not bad.well_formed()
    for fn in (q8_raw_count, q8_raw_blocks):
        with pytest.raises(ValueError):
            fn(bad)
    # every distinct layout is another key: the caches keep only the latest few
    for i in range(3 * arena._Q8_CACHE):
        lay = ParamLayout(("b",), ((64 * (i + 1),),), ("float32",), (0,), 64 * (i + 1))
        assert arena.q8_raw_table(lay, "cpu").tolist() == list(range(i + 1))
    assert len(arena._Q8_RAW) <= arena._Q8_CACHE and len(arena._Q8_RAW_TABLES) <= arena._Q8_CACHE


def test_xgmi_receiver_refuses_a_q8_header_that_does_not_match_the_layout(q8_wire, monkeypatch):
    """Unknown encoding, wrong raw count, a size one byte off either way, a wrong
    element type: each is answered with a wnack before a receive is reserved."""
    import msgpack

    from p2pfl_amd.communication.xgmi import XgmiSimNetwork
    from p2pfl_amd.data import MnistFederatedDM
    from p2pfl_amd.node import Node
    from p2pfl_amd.utils import wait_convergence

    net = XgmiSimNetwork()
    nodes = [Node(MLP(seed=i), MnistFederatedDM(sub_id=i, number_sub=400), protocol=net.protocol, device="cpu")
             for i in range(2)]
    for nd in nodes:
        nd.start()
    try:
        nodes[1].connect(nodes[0].addr)
        wait_convergence(nodes, 1, only_direct=True, wait=10)
        recv, send = nodes[0]._communication_protocol, nodes[1]._communication_protocol
        assert recv.plane.ready.wait(10)
        recv._server.commands["probe"] = object()  # a command without a precheck
        layout = flatten(MLP().state_dict()).layout
        layout_s = json.dumps(layout.to_json(), separators=(",", ":"))
        n_raw = len(q8_raw_blocks(layout))
        size = ops.q8_packed_nbytes(layout.numel, n_raw)
        sent = []
        monkeypatch.setattr(recv.bus, "send", lambda dst, data: sent.append((dst, msgpack.unpackb(data, raw=False))))
        base = {"ep": 0, "gen": recv.plane.gen, "n": size, "dt": "uint8", "rk": 1, "enc": "q8", "raw": n_raw}
        bad = [dict(base, enc="q4"), dict(base, raw=n_raw + 1), dict(base, n=size - 1), dict(base, n=size + 1),
               dict(base, dt="float32")]
        for i, hdr in enumerate(bad):
            hdr["seq"] = 100 + i
            recv._on_wput(send.addr, ["wput", hdr, send.addr, 0, [f"c{i}"], 1, "probe", layout_s])
            dst, (kind, seq, reason, evict) = sent[-1]
            assert (dst, kind, seq, evict) == (send.addr, "wnack", 100 + i, False)
            assert "q8" in reason or "encoding" in reason
        assert len(sent) == len(bad) and recv.plane.stats["accepted"] == 0 and not recv._inbound
    finally:
        for nd in nodes:
            nd.stop()
