"""GPU: the forward 3x3x3 conv over a VIRTUAL concatenation of two tensors (ConvOpt::in1), one conv per body through the single-operator entry
point dffw_op_conv3d_cat (engine.op_conv3d_cat).  Five layers of the depth network run this way -- the three hourglass conv0
layers (8 + 8 -> 8, 16 + 16 -> 16, 32 + 32 -> 32) and the pyramid's combine1 / combine2 (64 + 64 -> 64, 128 + 64 -> 128) -- and every conv family
has a fill of its own for it: conv_rollx_pair, conv_rollx_k2, conv_rollk, conv_roll (pair and plain), conv_tile (lean, generic, teams, split-K),
conv_small and conv_igemm.  Each is held here

* per element to the forward-error bound of oracle/error_bounds.py against eb.conv_ref64 of torch.cat([xa, xb], 1) in float64, finite everywhere (the
  op's record workspace is poisoned with NaN) and to the relative-L2 tolerance of tests/test_gpu_ops.py;
* bit for bit to engine.op_conv3d of the materialised concatenation under the same switches: the filter fragments and the chunk order come from the
  packed layer alone, which sees only Ca + Cb, so the two forms differ in their fill and in nothing else -- in every family (read in conv_roll's and
  conv_rollx's per-wave source select, conv_rollk's per-piece descriptor, conv_tile's per-lane source select of issue_fill, the tap table of
  conv_igemm / conv_small).  No row is pair-bounded only; check_pair is held as well;
* with one source silent (xa = 0, then xb = 0): D then carries the live source's terms only, so a leak of the other source's filter columns is over
  the bound;
* through eb.REGIMES with each source drawn on its own: the impulse regime puts unit impulses into the first and last channel of EACH source, on both
  sides of the concat boundary, and the output must be exactly 0 wherever D == 0.

The inputs are non-zero, carry a per-slice offset and a different level per source (xa += 0.25 z, xb -= 0.25 z + 0.5), so a slice or a source read from
the wrong place is a wrong value.  The streaming rows run as tests/test_gpu_roll_stream.py runs the single-source forms: rolling kernels forced, eight
workgroups, whole slice ranges and two ranges per sample, the straight-line and the generic epilogue."""
import pytest
import torch

from oracle import error_bounds as eb
from test_gpu_ops import TOL, bn_params, bounded, family, ref64, rel, rnd
from test_gpu_ops import worst_ratio_report  # noqa: F401  (module-scoped autouse fixture: ERROR_BOUND_REPORT gets this module's ratios too)
from test_gpu_roll_stream import SHAPES, SWITCHES as ROLL_SWITCHES

pytestmark = pytest.mark.gpu

ALL3 = ("bf16x3", "fp16", "bf16")
X3 = ("bf16x3",)
PIDX = {"bf16x3": 0, "fp16": 1, "bf16": 2}
SWITCHES = tuple(ROLL_SWITCHES) + ("DFFW_ROLLK_MERGE_BELOW", "DFFW_NO_LEAN_TILE", "DFFW_TEAM_MAX_WGS", "DFFW_NO_TEAMS", "DFFW_NO_TILE", "DFFW_NO_ROLLK")
BASE = {"DFFW_ROLL_MIN_UNITS": "1", "DFFW_ROLL_WGS": "8"}
ROLLK_SHAPES = SHAPES + [(1, 1, 8, 8), (3, 4, 28, 36)]   # a single 8 x 8 column; partial columns at the bottom / right edge (predicated)

# (name, Ca, Cb, Cout, residual, relu, extra environment, kernel prefix (%d: the precision index), precisions, shapes, shape of the silent-source and regime cases)
STREAM_ROWS = [
    ("rollx_pair", 8, 8, 8, False, 1, {}, "dffw::conv_rollx_pair<", X3, SHAPES, (2, 2, 32, 64)),
    ("rollx_pair_norelu", 8, 8, 8, False, 0, {}, "dffw::conv_rollx_pair<", X3, SHAPES, (2, 2, 32, 64)),
    ("roll_pair_serial", 8, 8, 8, False, 1, {"DFFW_NO_ROLLX": "1"}, "dffw::conv_roll<%d, 8, 16, 4, 6, false, true,", ALL3, SHAPES, (2, 2, 32, 64)),
    ("roll_pair_res", 8, 8, 8, True, 1, {}, "dffw::conv_roll<%d, 8, 16, 4, 6, %s, true,", ALL3, SHAPES, (2, 2, 32, 64)),
    ("roll_plain", 8, 8, 16, False, 1, {}, "dffw::conv_roll<%d, 8, 16, 4, 6, false, false,", ALL3, SHAPES, (2, 2, 32, 64)),
    ("roll_plain_res", 8, 8, 16, True, 1, {}, "dffw::conv_roll<%d, 8, 16, 4, 6, %s, false,", ALL3, SHAPES, (2, 2, 32, 64)),
    ("rollx_k2", 16, 16, 16, False, 1, {}, "dffw::conv_rollx_k2<", X3, SHAPES, (2, 2, 32, 64)),
    ("rollx_k2_norelu", 16, 16, 16, False, 0, {}, "dffw::conv_rollx_k2<", X3, SHAPES, (2, 2, 32, 64)),
    ("rollk4_32", 16, 16, 32, False, 1, {}, "dffw::conv_rollk<4,", X3, ROLLK_SHAPES, (3, 4, 28, 36)),
    ("rollk4_32_res", 16, 16, 32, True, 1, {}, "dffw::conv_rollk<4,", X3, ROLLK_SHAPES, (3, 4, 28, 36)),
    ("rollk4_64", 16, 16, 64, False, 1, {}, "dffw::conv_rollk<4,", X3, ROLLK_SHAPES, (3, 4, 28, 36)),
    ("rollk4_64_res", 16, 16, 64, True, 1, {}, "dffw::conv_rollk<4,", X3, ROLLK_SHAPES, (3, 4, 28, 36)),
    ("rollk8_32", 32, 32, 32, False, 1, {}, "dffw::conv_rollk<8,", X3, ROLLK_SHAPES, (3, 4, 28, 36)),
    ("rollk8_32_res", 32, 32, 32, True, 1, {}, "dffw::conv_rollk<8,", X3, ROLLK_SHAPES, (3, 4, 28, 36)),
    ("rollk8_64", 32, 32, 64, False, 1, {}, "dffw::conv_rollk<8,", X3, ROLLK_SHAPES, (3, 4, 28, 36)),
    ("rollk8_64_res", 32, 32, 64, True, 1, {}, "dffw::conv_rollk<8,", X3, ROLLK_SHAPES, (3, 4, 28, 36)),
]

NOROLL = {"DFFW_NO_ROLL": "1"}
FEW = {"DFFW_ROLL_MIN_UNITS": "100000", "DFFW_NO_SMALL": "1"}
TEAMS = dict(FEW, DFFW_TEAM_MAX_WGS="100000")
TILE = ("dffw::conv_tile<",)
# (name, Ca, Cb, Cout, (B, N, H, W), residual, environment, kernel prefixes, what the kernel name must also say (or None))
TILE_ROWS = [
    ("tile_lean_8_8", 8, 8, 8, (1, 2, 40, 48), False, NOROLL, TILE, "lean"),              # dres4.conv0 off whole columns
    ("tile_generic_8_8", 8, 8, 8, (1, 2, 40, 48), True, dict(NOROLL, DFFW_NO_LEAN_TILE="1"), TILE, "generic"),
    ("tile_16_16", 16, 16, 16, (2, 3, 12, 20), False, NOROLL, TILE, None),
    ("tile_32_32", 32, 32, 32, (2, 3, 12, 20), True, NOROLL, TILE, None),
    ("tile_teams_64_64", 64, 64, 64, (2, 3, 8, 8), True, TEAMS, TILE, None),   # (the switch lifts the cap on a team launch's workgroups;
    ("tile_few_64_64", 64, 64, 64, (2, 3, 8, 8), True, FEW, TILE, None),
    ("tile_teams_128_64", 128, 64, 128, (2, 3, 8, 8), True, TEAMS, TILE, None),   # whether teams or split-K run is the layer's matter: the report's key says which)
    ("tile_few_128_64", 128, 64, 128, (2, 3, 8, 8), False, FEW, TILE, None),
    ("tile_ragged_128_64", 128, 64, 128, (1, 2, 12, 20), True, FEW, TILE, None),
    ("small_64_64", 64, 64, 64, (2, 3, 7, 5), True, {}, ("dffw::conv_small<",), None),
    # (192 -> 128 at 7 x 5 under default switches is conv_tile's: its 8-wide block fits the grid.  The gather family then needs DFFW_NO_TILE)
    ("tile_default_128_64", 128, 64, 128, (2, 3, 7, 5), False, {}, TILE, None),
    ("small_128_64", 128, 64, 128, (2, 3, 7, 5), False, {"DFFW_NO_TILE": "1"}, ("dffw::conv_small<",), None),
    ("igemm_64_64", 64, 64, 64, (2, 3, 7, 5), False, {"DFFW_NO_SMALL": "1", "DFFW_NO_TILE": "1"}, ("dffw::conv_igemm<",), None),
    ("igemm_128_64", 128, 64, 128, (2, 3, 7, 5), True, {"DFFW_NO_SMALL": "1", "DFFW_NO_TILE": "1"}, ("dffw::conv_igemm<",), None),
    # the mirror split: the engine never makes it, the dispatch admits it
    ("mirror_64_128", 64, 128, 128, (2, 3, 8, 8), True, {}, ("dffw::conv_tile<", "dffw::conv_small<", "dffw::conv_igemm<"), None),
]


@pytest.fixture(scope="module")
def eng(lib_built):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dffinthewild_amd import engine
    return engine


def _set(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def row_prefix(prefix, prec):
    """A row's kernel prefix in one arithmetic.  conv_roll's RES argument is the residual PREFETCH of the split-bf16 instantiations: the fp16 and
    bf16 ones read the residual in the generic epilogue and say ``false`` with or without one."""
    if "%s" in prefix:
        return prefix % (PIDX[prec], "true" if prec == "bf16x3" else "false")
    return prefix % PIDX[prec] if "%d" in prefix else prefix


def targs(kn):
    return [s.strip() for s in kn[kn.index("<") + 1:kn.rindex(">")].split(",")]


def label(kn):
    """The report's key of a two-source launch: the family, and the form within it (conv_rollk's wave count, conv_roll's pair form, conv_tile's variant)."""
    fam, t = family(kn), targs(kn)
    if fam == "conv_rollk":
        fam += t[0]
    elif fam == "conv_roll":
        fam += "_pair" if t[6] == "true" else "_plain"
    elif fam == "conv_tile":
        fam += "_teams" if int(t[-1]) > 1 else "_splitk" if t[-3] == "true" else "_lean" if t[-2] == "true" else "_generic"
    return "dffw::cat." + fam + "<"


def sources(B, ca, cb, N, H, W, silent=None):
    """Two non-zero tensors, every slice at its own level and the two sources at different ones; ``silent`` ("a" / "b"): that one all zeros."""
    z = torch.arange(1, N + 1, dtype=torch.float32).reshape(1, 1, N, 1, 1)
    xa = rnd(B, ca, N, H, W, seed=11) + 0.25 * z
    xb = rnd(B, cb, N, H, W, seed=15) - (0.25 * z + 0.5)
    if silent == "a":
        xa = torch.zeros_like(xa)
    if silent == "b":
        xb = torch.zeros_like(xb)
    return xa, xb


def weights(ca, cb, cout):
    return rnd(cout, ca + cb, 3, 3, 3, seed=12, scale=(2.0 / ((ca + cb) * 27)) ** 0.5 * 1.7), bn_params(cout, 13)


class Pair:
    """One case on the GPU: the op over (xa, xb) and op_conv3d over their materialised concatenation, same weights and epilogue."""

    def __init__(self, eng, xa, xb, w, bn, res, relu, prec):
        self.eng, self.w = eng, w
        self.xa, self.xb, self.xc = xa.cuda(), xb.cuda(), torch.cat([xa, xb], 1).cuda()
        self.kw = dict(bn=bn, residual=res.cuda() if res is not None else None, relu=relu, precision=prec)

    def cat(self):
        got = self.eng.op_conv3d_cat(self.xa, self.xb, self.w, **self.kw)
        return got, self.eng.last_conv_kernel()

    def single(self):
        alt = self.eng.op_conv3d(self.xc, self.w, pad=1, **self.kw)
        return alt, self.eng.last_conv_kernel()


def held(p, r, prec, prefixes, what):
    """The op's result under the current switches: the family it must report, the bound, the relative-L2 gate, and the bits of (and the family of)
    the single-source op on the concatenation.  -> (result, kernel name)"""
    got, kn = p.cat()
    assert kn.startswith(prefixes), (what, kn)
    assert got.shape == r.ref.shape
    bounded(got, r, prec, label(kn), what)
    assert rel(got, r.ref) <= TOL[prec], (what, kn, rel(got, r.ref))
    alt, ka = p.single()
    assert family(ka) == family(kn), (what, kn, ka)
    eb.check_pair(got, alt, r, prec, "%s: two sources vs their concatenation" % what)
    assert torch.equal(got, alt), (what, kn, ka, "the two-source form differs from the single-source form on the concatenation")
    return got, kn


def zeros_where_no_term(got, r, what, must_exist=False):
    zero = r.D == 0
    assert bool(zero.any()) or not must_exist, what
    assert torch.equal(got.cpu()[zero], torch.zeros(int(zero.sum()))), what


_STREAM = [(row, shape, prec) for row in STREAM_ROWS for shape in row[9] for prec in row[8]]


@pytest.mark.parametrize("row,shape,prec", _STREAM, ids=["%s-b%d_n%d_%dx%d-%s" % ((r[0],) + s + (p,)) for r, s, p in _STREAM])
def test_cat_stream(eng, row, shape, prec, monkeypatch):
    """The streaming families' two-source fill on the slice stream of test_roll_stream: every switch combination within the bound and equal to the
    single-source op bit for bit; the generic epilogue and two slice ranges per sample equal the lean one and whole ranges bit for bit."""
    name, ca, cb, cout, residual, relu, extra, prefix, _, _, _ = row
    B, N, H, W = shape
    prefix = row_prefix(prefix, prec)
    xa, xb = sources(B, ca, cb, N, H, W)
    w, bn = weights(ca, cb, cout)
    res = rnd(B, cout, N, H, W, seed=14) if residual else None
    r = ref64(("cat", ca, cb, cout, residual, relu, shape), torch.cat([xa, xb], 1), w, stride=1, pad=1, bn=bn, residual=res, relu=relu)
    p = Pair(eng, xa, xb, w, bn, res, relu, prec)
    base = dict(BASE, **extra)
    lean = whole = None
    for zsplit in (1, 2):
        if zsplit > N:
            continue
        for generic in (False, True):
            _set(monkeypatch, dict(base, DFFW_ROLL_ZSPLIT=str(zsplit), **({"DFFW_NO_LEAN_ROLL": "1"} if generic else {})))
            got, kn = held(p, r, prec, prefix, "%s zsplit %d %s" % (name, zsplit, "generic" if generic else "lean"))
            if prefix.startswith("dffw::conv_roll<"):   # the body with a straight-line epilogue (split-bf16 alone): the switch picks the instantiation
                assert kn.endswith("false>" if generic or prec != "bf16x3" else "true>"), (name, generic, kn)
            if not generic:
                lean = got
            else:
                assert torch.equal(got, lean), (name, zsplit, "the generic epilogue differs from the straight-line one")
        if zsplit == 1:
            whole = lean
        else:   # a range boundary inside the volume changes which steps are dead, never a value
            assert torch.equal(lean, whole), (name, "two slice ranges per sample differ from whole ranges")
    if prefix.startswith("dffw::conv_rollk<8") and cout == 64:   # the two 32-channel output halves as two launches instead of grid.y = 2 of one
        _set(monkeypatch, dict(base, DFFW_ROLLK_MERGE_BELOW="1"))
        two, _ = held(p, r, prec, prefix, "%s two launches" % name)
        assert torch.equal(two, whole), (name, "two launches differ from one")


_SILENT = [(row, prec, s) for row in STREAM_ROWS for prec in row[8] for s in ("a", "b")]


@pytest.mark.parametrize("row,prec,silent", _SILENT, ids=["%s-%s-x%s_zero" % (r[0], p, s) for r, p, s in _SILENT])
def test_cat_stream_one_source_silent(eng, row, prec, silent, monkeypatch):
    """One source all zeros: the bound's scale D carries the live source's products only, so the other source's filter columns, or a poisoned piece
    of the ring, reaching an output is over the bound."""
    name, ca, cb, cout, residual, relu, extra, prefix, _, _, shape = row
    B, N, H, W = shape
    prefix = row_prefix(prefix, prec)
    xa, xb = sources(B, ca, cb, N, H, W, silent)
    w, bn = weights(ca, cb, cout)
    res = rnd(B, cout, N, H, W, seed=14) if residual else None
    r = ref64(("cat_silent", ca, cb, cout, residual, relu, shape, silent), torch.cat([xa, xb], 1), w, stride=1, pad=1, bn=bn, residual=res, relu=relu)
    _set(monkeypatch, dict(BASE, DFFW_ROLL_ZSPLIT="2", **extra))
    got, _ = held(Pair(eng, xa, xb, w, bn, res, relu, prec), r, prec, prefix, "%s x%s = 0" % (name, silent))
    zeros_where_no_term(got, r, name)


def regime_case(regime, ca, cb, cout, shape, residual, relu):
    """Each source drawn on its own in the regime, the BatchNorm of the regime; the impulse regime keeps a residual row's residual, as zeros (the
    instantiation stays the row's, and D == 0 outside the footprints)."""
    B, N, H, W = shape
    xa, xb = eb.regime_input(regime, (B, ca, N, H, W), seed=101), eb.regime_input(regime, (B, cb, N, H, W), seed=105)
    w = rnd(cout, ca + cb, 3, 3, 3, seed=102, scale=(2.0 / ((ca + cb) * 27)) ** 0.5 * 1.7)
    conv_mean = 3.0 * float(w.sum()) / cout if regime == "offset" else 0.0   # (both sources carry the offset: the whole filter)
    bn = eb.bn_regime(regime, cout, 103, conv_mean=conv_mean)
    res = None
    if residual:
        res = torch.zeros(B, cout, N, H, W) if regime == "impulse" else rnd(B, cout, N, H, W, seed=104)
    r = ref64(("cat_regime", regime, ca, cb, cout, residual, relu, shape), torch.cat([xa, xb], 1), w, stride=1, pad=1, bn=bn, residual=res, relu=relu)
    assert float(r.ref.abs().max()) < 1e4
    return xa, xb, w, bn, res, r


_STREAM_RG = [(row, rg, prec) for row in STREAM_ROWS for rg in eb.REGIMES for prec in row[8]]


@pytest.mark.parametrize("row,regime,prec", _STREAM_RG, ids=["%s-%s-%s" % (r[0], g, p) for r, g, p in _STREAM_RG])
def test_cat_stream_regimes(eng, row, regime, prec, monkeypatch):
    """The streaming rows on the inputs and BatchNorm statistics of test_conv_kernels_wide_regimes, each source drawn on its own."""
    name, ca, cb, cout, residual, relu, extra, prefix, _, _, shape = row
    prefix = row_prefix(prefix, prec)
    xa, xb, w, bn, res, r = regime_case(regime, ca, cb, cout, shape, residual, relu)
    _set(monkeypatch, dict(BASE, DFFW_ROLL_ZSPLIT="2", **extra))
    got, _ = held(Pair(eng, xa, xb, w, bn, res, relu, prec), r, prec, prefix, "%s %s" % (name, regime))
    zeros_where_no_term(got, r, (name, regime), must_exist=regime == "impulse")


def tile_form(kn, prec, form, what):
    if family(kn) != "conv_tile" or form is None:
        return
    lean = form == "lean" and prec == "bf16x3"   # (..., SPLITK, LEAN, KT>): LEAN exists in split-bf16 alone
    assert kn.endswith(", false, %s, 1>" % ("true" if lean else "false")), (what, kn)


_TILE = [(row, prec) for row in TILE_ROWS for prec in ALL3]


@pytest.mark.parametrize("row,prec", _TILE, ids=["%s-%s" % (r[0], p) for r, p in _TILE])
def test_cat_tile_and_gather(eng, row, prec, monkeypatch, capsys):
    """conv_tile (lean, generic, teams, few-tile), conv_small and conv_igemm over two sources, all three arithmetics; then each source silent."""
    name, ca, cb, cout, shape, residual, env, prefixes, form = row
    B, N, H, W = shape
    w, bn = weights(ca, cb, cout)
    res = rnd(B, cout, N, H, W, seed=14) if residual else None
    _set(monkeypatch, env)
    for silent in (None, "a", "b"):
        xa, xb = sources(B, ca, cb, N, H, W, silent)
        r = ref64(("cat_tile", name, silent), torch.cat([xa, xb], 1), w, stride=1, pad=1, bn=bn, residual=res, relu=1)
        what = name if silent is None else "%s x%s = 0" % (name, silent)
        got, kn = held(Pair(eng, xa, xb, w, bn, res, 1, prec), r, prec, prefixes, what)
        tile_form(kn, prec, form, what)
        zeros_where_no_term(got, r, what)
    with capsys.disabled():
        print("\n  %s %s: %s" % (name, prec, kn))


_TILE_RG = [(row, rg, prec) for row in TILE_ROWS for rg in eb.REGIMES for prec in ALL3]


@pytest.mark.parametrize("row,regime,prec", _TILE_RG, ids=["%s-%s-%s" % (r[0], g, p) for r, g, p in _TILE_RG])
def test_cat_tile_and_gather_regimes(eng, row, regime, prec, monkeypatch):
    name, ca, cb, cout, shape, residual, env, prefixes, form = row
    xa, xb, w, bn, res, r = regime_case(regime, ca, cb, cout, shape, residual, 1)
    _set(monkeypatch, env)
    got, kn = held(Pair(eng, xa, xb, w, bn, res, 1, prec), r, prec, prefixes, "%s %s" % (name, regime))
    tile_form(kn, prec, form, (name, regime))
    zeros_where_no_term(got, r, (name, regime), must_exist=regime == "impulse")


def test_wrapper_refusals_on_the_gpu(eng):
    """What the library refuses comes back as ValueError with its message; nothing was launched."""
    xa = torch.zeros(1, 8, 2, 8, 16, device="cuda")
    w = torch.zeros(8, 16, 3, 3, 3)
    for bad_a, bad_b, bad_w in ((xa[:, :4], xa, torch.zeros(8, 12, 3, 3, 3)), (xa, xa.repeat(1, 24, 1, 1, 1), torch.zeros(8, 200, 3, 3, 3)),
                                (xa, xa, torch.zeros(136, 16, 3, 3, 3)), (xa, xa, torch.zeros(12, 16, 3, 3, 3))):
        with pytest.raises(ValueError):
            eng.op_conv3d_cat(bad_a, bad_b, bad_w)
    with pytest.raises(ValueError):
        eng.op_conv3d_cat(xa, xa, w, precision="bf16x3", residual=torch.zeros(1, 8, 2, 8, 8, device="cuda"))
    assert torch.equal(eng.op_conv3d_cat(xa, xa, w), torch.zeros(1, 8, 2, 8, 16, device="cuda"))
