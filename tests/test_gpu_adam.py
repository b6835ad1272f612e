"""The Adam step on the GPU: every element of p, m and v against the float64 formulas of tests/adam_ref.py under its
per-element bounds: sizes and tails around the chunk between poisoned gaps; each pointer off a 16-byte boundary, bit-identical to the aligned
run; lists below, at and beyond the launch's capacity, each tensor bit-identical to passing it alone; the four regimes over t and lr; two runs
and a side stream; five steps through pipeline.Adam, each held to the state the GPU itself left; checkpoints to torch.optim.Adam and back;
three training steps of the real head chain conv3d -> batch_norm3d -> score_conv -> HeadsLoss.

Every case prints its worst err / bound (pytest -s); DESIGN.md section 20 is where the table of them goes."""
import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adam_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KERNEL = "dffw::adam_kernel"
CHUNK = 4096            # ADAM_CHUNK of csrc/dffw_optim.h: elements per workgroup
GAP = 64                # floats between two carved tensors
POISON = 0x7FC0BAD1     # a NaN
SMALL = [1, 2, 3, 4, 5, 7, 8, 255, 256, 257]
SIZES = SMALL + [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3, 65539]


@pytest.fixture(scope="module")
def eng(lib_built):
    from dffinthewild_amd import engine
    return engine


class Carved:
    """Tensors of ``sizes`` carved out of one GPU buffer per role (p, g, m, v), each starting ``offsets[role]`` floats after a 16-byte boundary,
    with at least GAP floats of POISON in front of, between and behind them; filled from the elements of ``case`` in order."""

    def __init__(self, sizes, case, offsets=(0, 0, 0, 0)):
        self.sizes, self.case = list(sizes), case
        assert sum(sizes) == case["p"].numel()
        self.buf, self.views, self.host = {}, {}, {}
        for role, off in zip("pgmv", offsets):
            spans, pos = [], GAP
            for n in sizes:
                start = (pos + 3) // 4 * 4 + off
                spans.append((start, start + n))
                pos = start + n + GAP
            host = torch.full((pos,), POISON, dtype=torch.int32).view(torch.float32)
            at = 0
            for (a, b) in spans:
                host[a:b] = case[role][at:at + b - a]
                at += b - a
            self.host[role] = host
            self.buf[role] = host.cuda()
            assert self.buf[role].data_ptr() % 16 == 0
            self.views[role] = [self.buf[role][a:b] for (a, b) in spans]
            assert all(v.data_ptr() % 16 == 4 * off for v in self.views[role])
            setattr(self, "spans_" + role, spans)

    def lists(self):
        return [self.views[r] for r in "pgmv"]

    def run(self, eng):
        eng.op_adam_step(*self.lists(), step=self.case["t"], lr=self.case["lr"], betas=self.case["betas"], eps=self.case["eps"])
        torch.cuda.synchronize()
        return self

    def got(self):
        return {k: torch.cat([v.cpu() for v in self.views[r]]) for k, r in (("p", "p"), ("m", "m"), ("v", "v"))}

    def check_untouched(self):
        """The gaps of p, m and v and the whole of g: the bits they had."""
        assert R.same_bits(self.buf["g"], self.host["g"]), "grad was written"
        for role in "pmv":
            now = self.buf[role].cpu().view(torch.int32)
            gap = torch.ones(now.numel(), dtype=torch.bool)
            for (a, b) in getattr(self, "spans_" + role):
                gap[a:b] = False
            assert bool((now[gap] == POISON).all()), "%s: %d gap words were written" % (role, int((now[gap] != POISON).sum()))


def test_sizes_and_tails_between_poisoned_gaps(eng):
    """One call over 1 .. 8, 255 .. 257, the chunk - 1 / exact / + 1, two chunks + 3 and 65 539 elements: vector bodies, tails of 0 .. 3, the
    last chunk of one element."""
    case = R.make_case("plain", sum(SIZES), 10, 1e-1, seed=1)
    c = Carved(SIZES, case).run(eng)
    assert eng.op_kernels() == [KERNEL]
    w = R.check(c.got(), case, "sizes")
    print("sizes and tails: worst err/bound p %.3f m %.3f v %.3f" % (w["p"], w["m"], w["v"]))
    c.check_untouched()


def test_each_pointer_off_a_16_byte_boundary(eng):
    """The element-wise path: each of param, grad, exp_avg, exp_avg_sq in turn 4, 8 and 12 bytes past a 16-byte boundary, the others on one.
    Within the bound, gaps and grad untouched, and the bits of the aligned run of the same values."""
    sizes = SMALL + [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
    case = R.make_case("plain", sum(sizes), 10, 1e-1, seed=2)
    aligned = Carved(sizes, case).run(eng)
    base = aligned.got()
    R.check(base, case, "aligned")
    worst = 0.0
    for role in range(4):
        for off in (1, 2, 3):
            offsets = [0, 0, 0, 0]
            offsets[role] = off
            c = Carved(sizes, case, offsets).run(eng)
            got = c.got()
            worst = max(worst, *R.check(got, case, "role %d offset %d" % (role, off)).values())
            c.check_untouched()
            for k in "pmv":
                assert R.same_bits(got[k], base[k]), "%s differs from the aligned run with pointer %d offset by %d floats" % (k, role, off)
    print("misaligned pointers: worst err/bound %.3f, bit-identical to the aligned run" % worst)


def _list_tensors(n, case):
    """n GPU tensors per role, sizes cycling through 8, 27 * 8 * 8 and 1, each an allocation of its own; values from ``case`` in order."""
    sizes = [(8, 27 * 8 * 8, 1)[i % 3] for i in range(n)]
    out, at = {r: [] for r in "pgmv"}, 0
    for s in sizes:
        for r in "pgmv":
            out[r].append(case[r][at:at + s].clone().cuda())
        at += s
    return sizes, out


def test_list_lengths_and_launches(eng):
    """1, L, L + 1 and 2 L + 3 tensors (L = ADAM_TENSORS_PER_LAUNCH): ceil(n / L) launches, each tensor bit-identical to passing it alone (it
    is then entry 0 of a launch of its own), an empty tensor in the middle skipped."""
    L = eng.ADAM_TENSORS_PER_LAUNCH
    nmax = 2 * L + 3
    total = sum((8, 27 * 8 * 8, 1)[i % 3] for i in range(nmax))
    case = R.make_case("plain", total, 3, 1e-2, seed=3)
    kw = dict(step=case["t"], lr=case["lr"], betas=case["betas"], eps=case["eps"])
    _, alone = _list_tensors(nmax, case)
    for i in range(nmax):
        eng.op_adam_step(*[[alone[r][i]] for r in "pgmv"], **kw)
        assert eng.op_kernels() == [KERNEL]
    torch.cuda.synchronize()
    R.check({k: torch.cat([t.cpu() for t in alone[k]]) for k in "pmv"}, case, "alone")
    for n in (1, L, L + 1, nmax):
        for with_empty in (False, True):
            sizes, t = _list_tensors(n, case)
            lists = [list(t[r]) for r in "pgmv"]
            if with_empty:
                for l in lists:
                    l.insert(n // 2, torch.empty(0).cuda())
            eng.op_adam_step(*lists, **kw)
            assert eng.op_kernels() == [KERNEL] * ((n + L - 1) // L), (n, with_empty, eng.op_kernels())
            torch.cuda.synchronize()
            for i in range(n):
                for r in "pmv":
                    assert R.same_bits(t[r][i], alone[r][i]), "tensor %d of %d (%s): not the bits of passing it alone" % (i, n, r)
                assert R.same_bits(t["g"][i], alone["g"][i])
    print("lists of 1, %d, %d, %d tensors: every tensor bit-identical to passing it alone" % (L, L + 1, nmax))


def test_regimes(eng):
    """All CASES x t x lr at 4 099 elements (a chunk and a tail of 3).  Prints the worst ratios per regime, and how many elements carry exactly
    the bits of the fp32 emulation of the kernel's operation order."""
    worst, same, count = {}, 0, 0
    for case in R.all_cases(CHUNK + 3, seed=4):
        t = {r: case[r].clone().cuda() for r in "pgmv"}
        eng.op_adam_step([t["p"]], [t["g"]], [t["m"]], [t["v"]], step=case["t"], lr=case["lr"], betas=case["betas"], eps=case["eps"])
        got = {k: t[k].cpu() for k in "pmv"}
        assert R.same_bits(t["g"], case["g"])
        w = R.worst_ratio(got, case)
        for k in "pmv":
            worst[case["regime"], k] = max(worst.get((case["regime"], k), 0.0), w[k])
        emu = R.emulate(case)
        same += sum(int((got[k].view(torch.int32) == emu[k].view(torch.int32)).sum()) for k in "pmv")
        count += 3 * got["p"].numel()
    for regime in R.CASES:
        print("%-10s worst err/bound  p %.3f  m %.3f  v %.3f" % ((regime,) + tuple(worst[regime, k] for k in "pmv")))
    print("%d of %d results carry the bits of the fp32 emulation" % (same, count))
    assert all(x <= 1.0 for x in worst.values()), worst


def test_two_runs_and_a_side_stream(eng):
    sizes = [5, CHUNK + 1, 3 * CHUNK + 2, 27 * 8 * 8]
    case = R.make_case("plain", sum(sizes), 7, 1e-2, seed=5)
    first = Carved(sizes, case).run(eng).got()
    R.check(first, case, "first run")
    second = Carved(sizes, case).run(eng).got()
    c = Carved(sizes, case)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eng.op_adam_step(*c.lists(), step=case["t"], lr=case["lr"], betas=case["betas"], eps=case["eps"])
    s.synchronize()
    side = c.got()
    c.check_untouched()
    for k in "pmv":
        assert R.same_bits(first[k], second[k]), "%s: two runs differ" % k
        assert R.same_bits(first[k], side[k]), "%s: the side stream's result differs" % k


def _snapshot(opt, params):
    """[(p, g, m, v)] on the CPU for the parameters that have a gradient: the state before a step (zeros where there is none yet)."""
    snap = []
    for p in params:
        if p.grad is None:
            snap.append(None)
            continue
        st = opt.state.get(p, {})
        m = st["exp_avg"].detach().cpu().clone() if "exp_avg" in st else torch.zeros(p.shape)
        v = st["exp_avg_sq"].detach().cpu().clone() if "exp_avg_sq" in st else torch.zeros(p.shape)
        snap.append((p.detach().cpu().clone(), p.grad.detach().cpu().contiguous().clone(), m, v))
    return snap


def _check_step(opt, params, snap, t, lr, what):
    """Every parameter's p, m, v after a step against the float64 reference evaluated from ``snap``."""
    worst = {k: 0.0 for k in "pmv"}
    for i, (p, s) in enumerate(zip(params, snap)):
        if s is None:
            continue
        case = dict(p=s[0].reshape(-1), g=s[1].reshape(-1), m=s[2].reshape(-1), v=s[3].reshape(-1), t=t, lr=lr, betas=R.BETAS, eps=R.EPS, regime=what)
        st = opt.state[p]
        got = dict(p=p.detach().cpu().reshape(-1), m=st["exp_avg"].cpu().reshape(-1), v=st["exp_avg_sq"].cpu().reshape(-1))
        w = R.check(got, case, "%s parameter %d step %d" % (what, i, t))
        worst = {k: max(worst[k], w[k]) for k in "pmv"}
    return worst


def test_five_steps_through_the_optimizer(eng):
    """pipeline.Adam over five parameters -- one without a gradient, one whose gradient is not contiguous -- for five steps with fresh gradients:
    each step against the reference evaluated from the state the GPU produced in the step before; ``step`` counts 1 .. 5."""
    from dffinthewild_amd import pipeline
    gen = torch.Generator().manual_seed(6)
    shapes = [(8,), (32, 32, 3, 3, 3), (CHUNK + 3,), (6, 10), (16,)]
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).cuda()) for s in shapes]
    frozen = params[4].detach().clone()
    lr = 1e-2
    opt = pipeline.Adam(params, lr=lr)
    assert opt.defaults["betas"] == R.BETAS
    for t in range(1, 6):
        for i, p in enumerate(params[:4]):
            g = 0.1 * torch.randn(p.shape if i != 3 else (10, 6), generator=gen).cuda()
            p.grad = g if i != 3 else g.t()
        assert not params[3].grad.is_contiguous()
        snap = _snapshot(opt, params)
        assert opt.step() is None
        w = _check_step(opt, params, snap, t, lr, "five steps")
        print("step %d: worst err/bound p %.3f m %.3f v %.3f" % (t, w["p"], w["m"], w["v"]))
        for p in params[:4]:
            s = opt.state[p]["step"]
            assert s.device.type == "cpu" and s.dtype == torch.float32 and s.dim() == 0 and float(s) == t
    assert params[4] not in opt.state and R.same_bits(params[4], frozen)


@pytest.mark.parametrize("direction", ["ours_to_torch", "torch_to_ours"])
def test_checkpoints_move_between_the_two_classes(eng, direction):
    """Two steps with one class, its state_dict loaded into the other, one more step with each from the same state and gradients: both within
    the bound of the float64 reference."""
    from dffinthewild_amd import pipeline
    gen = torch.Generator().manual_seed(7)
    shapes = [(8,), (27 * 8 * 8,), (3, 5)]
    lr = 1e-2
    make = dict(ours=lambda ps: pipeline.Adam(ps, lr=lr), torch=lambda ps: torch.optim.Adam(ps, lr=lr, betas=R.BETAS, foreach=False))
    first, second = ("ours", "torch") if direction == "ours_to_torch" else ("torch", "ours")
    pa = [torch.nn.Parameter(torch.randn(s, generator=gen).cuda()) for s in shapes]
    a = make[first](pa)
    for t in (1, 2):
        for p in pa:
            p.grad = 0.1 * torch.randn(p.shape, generator=gen).cuda()
        a.step()
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    b = make[second](pb)
    b.load_state_dict(copy.deepcopy(a.state_dict()))
    for p, q in zip(pa, pb):
        assert float(b.state[q]["step"]) == 2.0 and b.state[q]["exp_avg"].data_ptr() != a.state[p]["exp_avg"].data_ptr()
        p.grad = 0.1 * torch.randn(p.shape, generator=gen).cuda()
        q.grad = p.grad.clone()
    for name, opt, ps in ((first, a, pa), (second, b, pb)):
        snap = _snapshot(opt, ps)
        opt.step()
        torch.cuda.synchronize()
        w = _check_step(opt, ps, snap, 3, lr, "%s: %s" % (direction, name))
        print("%s, third step by %s: worst err/bound p %.3f m %.3f v %.3f" % (direction, name, w["p"], w["m"], w["v"]))
        assert all(float(opt.state[p]["step"]) == 3.0 for p in ps)


def test_training_the_real_head_chain(eng):
    """conv3d (32 -> 32, 3x3x3) -> batch_norm3d(relu) -> score_conv (32 -> 1, 1x1x1) -> HeadsLoss on a (1, 32, 4, 16, 16) volume, three steps of
    pipeline.Adam over the conv weight, gamma, beta and the score weight: each update held to the bound from the (p, g, m, v) snapshot taken
    before it; a parameter outside the graph is not touched.  The loss is printed, not gated."""
    from dffinthewild_amd import pipeline
    gen = torch.Generator().manual_seed(8)
    B, C, N, H, W = 1, 32, 4, 16, 16
    x = torch.randn(B, C, N, H, W, generator=gen).cuda()
    fd = (0.1 + 1.4 * torch.rand(B, N, 1, 1, generator=gen)).cuda()
    gt = (0.1 + 1.4 * torch.rand(B, H, W, generator=gen)).cuda()
    mask = (torch.rand(B, H, W, generator=gen) < 0.7).cuda()
    w = torch.nn.Parameter((0.05 * torch.randn(C, C, 3, 3, 3, generator=gen)).cuda())
    gamma = torch.nn.Parameter((1 + 0.1 * torch.randn(C, generator=gen)).cuda())
    beta = torch.nn.Parameter((0.1 * torch.randn(C, generator=gen)).cuda())
    ws = torch.nn.Parameter((0.2 * torch.randn(1, C, 1, 1, 1, generator=gen)).cuda())
    unused = torch.nn.Parameter(torch.randn(24, generator=gen).cuda())
    before = unused.detach().clone()
    params = [w, gamma, beta, ws, unused]
    lr = 1e-3
    opt = pipeline.Adam(params, lr=lr)
    for t in (1, 2, 3):
        opt.zero_grad()
        y = pipeline.conv3d(x, w, stride=1, pad=1)
        z = pipeline.batch_norm3d(y, gamma, beta, relu=True)
        s = pipeline.score_conv(z, ws, pad=0)
        total = pipeline.HeadsLoss.apply(s, s, s, s, fd, gt, mask)
        total.backward()
        assert all(p.grad is not None and p.grad.is_cuda and p.grad.shape == p.shape for p in params[:4]) and unused.grad is None
        snap = _snapshot(opt, params)
        opt.step()
        wr = _check_step(opt, params, snap, t, lr, "head chain")
        print("head chain step %d: loss %.6f, worst err/bound p %.3f m %.3f v %.3f" % (t, float(total.detach()), wr["p"], wr["m"], wr["v"]))
    assert unused not in opt.state and R.same_bits(unused, before)
