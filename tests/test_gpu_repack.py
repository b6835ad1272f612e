"""Repacking the weights on the GPU: an engine updated in place holds, bit for bit, what a newly built one holds.

Every comparison is torch.equal on bytes: the packed device buffers (Engine.packed_bytes: every layout of every layer, also those no small
forward dispatches to), the forward's outputs and score taps, and the same through Network and pipeline.Adam.  State dicts come from
synth.state_dict_numpy; the second one carries, in every conv weight and every BatchNorm, the values on which a device fold could part from the
host's: signed zeros, a float32 subnormal, a float whose bf16 rounding carries into the exponent, a float16 subnormal; running_var 0 and
1e-12, a negative and a zero gamma, a large running_mean; a -0.0 conv bias."""
import numpy as np
import pytest
import torch

from dffinthewild_amd import graph, synth

pytestmark = pytest.mark.gpu

NETS = ("depth", "e2e")
PRECS = ("bf16x3", "fp16", "bf16")
CARRY = np.array([0x3F7FFFFF], dtype=np.uint32).view(np.float32)[0]    # 1 - 2^-24: rounds up to 1.0 in bf16
SPECIAL = np.array([0.0, -0.0, 1e-39, CARRY, 6e-8], dtype=np.float32)

# one layer of each geometry the issue names; every other conv and BatchNorm carries the same values
GEOMETRY = {
    "stem": "DFF_net.FM_measure.Focus_extraction.0.0",
    "1x3x3": "DFF_net.FM_conv1.1.Focus_Measure.conv.0.0",
    "3x3x3": "DFF_net.dres0.0.0",
    "3x3x3 s(1,2,2)": "DFF_net.FM_conv1.0.stride_conv.0",
    "transposed": "DFF_net.deconv_1.0",
    "3x1x1": "DFF_net.FM_conv2.1.N_ch_attention.0",
    "1x1x1": "DFF_net.FM_conv2.1.N_ch_attention.2",
    "folded shortcut": "optical_flow_aggregation.OF_feature.1.feature",
    "head split": "optical_flow_aggregation.conv1.0.0",
    "biased head conv": "optical_flow_aggregation.conv3.6",
}


def _entries(net):
    return list(graph.param_entries(graph.e2e_convs() if net == "e2e" else graph.dff_net_convs()))


def _plant(sd):
    """The special values, scattered: every 53rd element of every conv weight in turn (closer in filters below 318 elements), five channels
    of every BatchNorm."""
    for key, v in sd.items():
        if v.ndim == 5:
            flat = v.reshape(-1)
            at = np.arange(3, flat.size, 53 if flat.size >= 6 * 53 else max(1, flat.size // 12))   # (the small filters: all five values too)
            flat[at] = SPECIAL[np.arange(at.size) % SPECIAL.size]
        elif key.endswith(".running_var"):
            v[0], v[1] = 0.0, 1e-12
        elif key.endswith(".running_mean"):
            v[4] = 1.0e4
        elif key.endswith(".1.weight") and v.ndim == 1:   # BatchNorm gamma
            v[2], v[3] = -0.7, 0.0
        elif key.endswith(".bias") and not key.endswith(".1.bias"):   # conv bias
            v[0] = -0.0
    return sd


_SD = {}


def state(net, which):
    """{name: CPU tensor}: 'a' plain, 'b' another seed with the special values planted."""
    if (net, which) not in _SD:
        sd = synth.state_dict_numpy(_entries(net), seed=11 if which == "a" else 12)
        sd = {k: np.array(v) for k, v in sd.items()}
        if which == "b":
            _plant(sd)
            for what, name in GEOMETRY.items():
                if name + ".weight" in sd:
                    w = sd[name + ".weight"].reshape(-1).view(np.uint32)
                    assert all((w == s.view(np.uint32)).any() for s in SPECIAL), what
        _SD[net, which] = {k: torch.from_numpy(v) for k, v in sd.items()}
    return _SD[net, which]


def on_gpu(sd):
    return {k: v.cuda() for k, v in sd.items()}


_CASES = {}


def case(net, prec):
    """Built once per (net, precision): Engine(a) and its bytes, the same engine updated to b and its bytes, a new Engine(b) and its bytes."""
    from dffinthewild_amd import engine
    if (net, prec) not in _CASES:
        which = engine.NET_E2E if net == "e2e" else engine.NET_DEPTH
        dev = torch.device("cuda", torch.cuda.current_device())
        c = {"b_gpu": on_gpu(state(net, "b")), "a_gpu": on_gpu(state(net, "a"))}
        c["upd"] = engine.Engine(state(net, "a"), dev, prec, which)
        c["bytes_a"] = c["upd"].packed_bytes()
        c["upd"].update(c["b_gpu"])
        c["bytes_upd"] = c["upd"].packed_bytes()
        c["new"] = engine.Engine(state(net, "b"), dev, prec, which)
        c["bytes_b"] = c["new"].packed_bytes()
        _CASES[net, prec] = c
    return _CASES[net, prec]


def _bits_equal(a, b):
    """Equal bit patterns (torch.equal on the floats would call two equal NaNs different)."""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _same(a, b, what):
    assert a.shape == b.shape, what
    if not torch.equal(a, b):
        diff = (a != b).nonzero().reshape(-1)
        raise AssertionError("%s: %d of %d bytes differ, first at %d" % (what, diff.numel(), a.numel(), int(diff[0])))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("net", NETS)
def test_every_buffer_every_layout(net, prec):
    c = case(net, prec)
    assert c["bytes_b"].dtype == torch.uint8 and c["bytes_b"].numel() > 1 << 20
    assert not torch.equal(c["bytes_a"], c["bytes_b"])
    _same(c["bytes_upd"], c["bytes_b"], "%s %s: updated engine vs a new one" % (net, prec))


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("net", NETS)
def test_no_residue_no_drift(net, prec):
    c = case(net, prec)
    e = c["upd"]
    e.update(c["b_gpu"])
    _same(e.packed_bytes(), c["bytes_b"], "second update to b")
    e.update(c["a_gpu"])
    _same(e.packed_bytes(), c["bytes_a"], "b then a vs a new Engine(a)")
    e.update(c["b_gpu"])
    _same(e.packed_bytes(), c["bytes_b"], "back to b")


def _inputs(net):
    if net == "e2e":
        B, N, H, W = 1, 10, 64, 64
    else:
        B, N, H, W = 1, 3, 32, 32
    FS = torch.from_numpy(synth.focal_stack(B, N, H, W, seed=5)).cuda()
    fd = torch.from_numpy(synth.focus_dists(B, N, 1, 1)).cuda()
    fov = (1.0 + 0.06 * torch.arange(N - 1, -1, -1, dtype=torch.float32) / (N - 1)).reshape(1, 1, N, 1, 1).cuda()
    return FS, fd, fov


TAPS = ["conf", "cost1", "cost2", "cost3"]


@pytest.mark.parametrize("net", NETS)
def test_forward_bits(net):
    c = case(net, "bf16x3")
    FS, fd, fov = _inputs(net)
    res = []
    for e in (c["upd"], c["new"]):
        outs, taps = e.forward_e2e(FS, fd, fov, taps=TAPS) if net == "e2e" else e.forward(FS, fd, taps=TAPS)
        res.append(list(outs) + [taps[k] for k in TAPS])
    torch.cuda.synchronize()
    for i, (u, n) in enumerate(zip(*res)):
        assert _bits_equal(u, n), "output / tap %d of the updated engine differs from the new engine's" % i


def _network(net, sd):
    if net == "e2e":
        from dffinthewild_amd.End_to_End import Network
    else:
        from dffinthewild_amd.Depth_Estimation_Network import Network
    m = Network()
    m.load_state_dict(sd)
    return m.cuda().eval()


def _call(model, net, inp):
    FS, fd, fov = inp
    with torch.no_grad():
        return model(FS, fd, fov) if net == "e2e" else model(FS, fd)


def _engine_of(model):
    return model._engines[torch.cuda.current_device()][1]


def _equal_to_new_network(model, net, inp, what):
    got = _call(model, net, inp)
    ref = _call(_network(net, {k: v.detach().cpu().float() if torch.is_floating_point(v) else v.cpu() for k, v in model.state_dict().items()}), net, inp)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert _bits_equal(g, r), "%s: output %d differs from a new Network with these parameters" % (what, i)
    return got


@pytest.mark.parametrize("net", NETS)
def test_through_network(net):
    inp = _inputs(net)
    model = _network(net, state(net, "a"))
    first = _call(model, net, inp)
    e0 = _engine_of(model)
    sd_b = state(net, "b")
    with torch.no_grad():
        for k, t in model.state_dict(keep_vars=True).items():
            if torch.is_floating_point(t):
                t.copy_(sd_b[k])
    got = _equal_to_new_network(model, net, inp, "in-place change")
    assert _engine_of(model) is e0, "an in-place change must go through Engine.update, not a rebuild"
    assert not _bits_equal(got[3], first[3])
    _same(e0.packed_bytes(), case(net, "bf16x3")["bytes_b"], "the Network's engine after the update")
    # load_state_dict: a new engine
    model.load_state_dict(state(net, "a"))
    again = _call(model, net, inp)
    assert _engine_of(model) is not e0
    assert all(_bits_equal(a, b) for a, b in zip(again, first))
    # a half-precision parameter: Engine.update would have to convert it, so the engine is rebuilt
    e1 = _engine_of(model)
    p = dict(model.named_parameters())["DFF_net.dres0.0.0.weight"]
    with torch.no_grad():
        p.data = p.data.half()
        dict(model.named_parameters())["DFF_net.dres0.2.0.weight"].mul_(0.5)
    _equal_to_new_network(model, net, inp, "a half-precision parameter")
    assert _engine_of(model) is not e1
    # invalidate(): a rebuild, too
    e2 = _engine_of(model)
    with torch.no_grad():
        p.data = p.data.float()
        p.mul_(1.5)
    model.invalidate()
    _equal_to_new_network(model, net, inp, "invalidate()")
    assert _engine_of(model) is not e2


def test_with_the_optimiser():
    """Three pipeline.Adam steps over every parameter with seeded gradients, a forward after each: the engine object stays, and each forward is
    a new Network's from a snapshot of the parameters."""
    from dffinthewild_amd import pipeline
    net = "depth"
    inp = _inputs(net)
    model = _network(net, state(net, "a"))
    _call(model, net, inp)
    e0 = _engine_of(model)
    params = [p for p in model.parameters() if torch.is_floating_point(p)]
    opt = pipeline.Adam(params, lr=1e-3)
    gen = torch.Generator().manual_seed(21)
    last = None
    for step in range(3):
        for p in params:
            p.grad = (0.05 * torch.randn(p.shape, generator=gen)).cuda()
        opt.step()
        got = _equal_to_new_network(model, net, inp, "Adam step %d" % (step + 1))
        assert _engine_of(model) is e0, "optimizer.step() must reach the engine through Engine.update"
        assert last is None or not _bits_equal(got[3], last[3])
        last = got


def test_refusals_leave_the_engine_as_it_was():
    from dffinthewild_amd import engine
    c = case("depth", "bf16x3")
    e = c["upd"]
    e.update(c["b_gpu"])
    before = e.packed_bytes()
    bn = "DFF_net.dres0.0.1.running_var"
    missing = {k: v for k, v in c["a_gpu"].items() if k != bn}
    with pytest.raises(engine.DffwError, match="no entry 'DFF_net.dres0.0.1.running_var'"):
        e.update(missing)
    short = dict(c["a_gpu"])
    short[bn] = short[bn][:-1].contiguous()
    with pytest.raises(ValueError, match="has 63 elements, expected 64"):
        e.update(short)
    host = dict(c["a_gpu"])
    host[bn] = host[bn].cpu()
    with pytest.raises(ValueError, match="is on cpu"):
        e.update(host)
    half = dict(c["a_gpu"])
    half[bn] = half[bn].half()
    with pytest.raises(ValueError, match="contiguous float32"):
        e.update(half)
    _same(e.packed_bytes(), before, "after four refused updates")


def test_enqueue_only_after_the_first_update():
    """The default stream is held busy by a chain of large matrix products; an update issued under a side stream returns while that chain
    still runs, allocates nothing, and gives the bytes of a new engine."""
    c = case("depth", "bf16x3")
    e = c["upd"]
    e.update(c["a_gpu"])          # (not the first update of this engine: its plan exists)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    a = torch.randn(8192, 8192, device="cuda")
    b = torch.mm(a, a)            # warm-up: the BLAS library's own first-call work
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    mem = torch.cuda.memory_allocated()
    for _ in range(40):
        torch.mm(a, a, out=b)
    done.record()
    with torch.cuda.stream(side):
        e.update(c["b_gpu"])
    returned_early = not done.query()
    assert torch.cuda.memory_allocated() == mem
    side.synchronize()
    torch.cuda.synchronize()
    assert returned_early, "Engine.update returned only after the default stream's work had finished"
    _same(e.packed_bytes(), c["bytes_b"], "update under a side stream")
