"""Zero-tolerance tests of the conv kernels: exactly representable operands, impulse probes, poisoned inputs.

The parity tests of test_gpu_kernels.py draw standard-normal operands and accept 2e-3 of the output scale.  Here the operands
are small integers: every product and every partial sum in any order is exact in fp32, so the fp32 sum is the float64
reference's value and every kernel family has to return the reference's BITS after one rounding to the output type.  The impulse
probes pin addressing (which input pixel, tap and channel reaches which output), the poison tests pin that nothing outside a
pixel's receptive field is read and then masked by a multiplication with zero (NaN / inf do not vanish that way).

tests/test_conv_exact_inputs.py imports the generator and the case lists from here and proves, without a device, that the
reference alone stays inside the conditions the bit comparison rests on.  Nothing device-specific is imported at module level.
"""
import collections
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# frp_conv2d_nhwc flag bits (include/frp.h; test_gpu_kernels.py establishes which kernel each combination runs)
BORDER, OUT_F32, RES_UP2 = 1, 2, 4
GENERIC, WINO, TILES_QUARTER, TILES_DEFAULT, NO_C64, S2 = 1 << 8, 1 << 16, 1 << 17, 1 << 18, 1 << 20, 1 << 21

Case = collections.namedtuple("Case", "N H W Cin Cout k stride act res flags ref_images")


def _case(N, H, W, Cin, Cout, k, stride, act, res, flags, ref_images=None):
    return Case(N, H, W, Cin, Cout, k, stride, act, res, flags, N if ref_images is None else min(N, ref_images))


# the smallest entries of test_gpu_kernels.py's lists (CONV_CASES, C64_CASES, S2_CASES, WINO_CASES / WINO_WIDE_CASES, F8_CASES)
GENERIC_CASES = [_case(*c) for c in [
    (1, 17, 13, 64, 128, 3, 2, 0, True, 0),
    (2, 9, 9, 128, 256, 1, 1, 2, False, 0),
    (1, 20, 20, 8, 32, 3, 2, 1, False, 0),
    (3, 7, 7, 256, 512, 3, 1, 2, False, 1),
    (1, 8, 8, 128, 128, 1, 1, 0, True, 4),
    (4, 1, 1, 1024, 512, 1, 1, 0, False, 2),
    (1, 5, 7, 64, 64, 3, 1, 1, True, 0),
    (1, 1, 1, 64, 64, 3, 1, 0, False, 0),
    (2, 19, 21, 64, 96, 3, 1, 0, False, 0),
]]
LEAN_CASES = [c for c in GENERIC_CASES if c.k == 3 and c.stride == 1 and c.Cin % 64 == 0] + [_case(*c) for c in [
    (1, 3, 300, 64, 64, 3, 1, 1, False, 0),
    (40, 7, 7, 128, 128, 3, 1, 2, True, 1),
    (70, 7, 7, 64, 64, 3, 1, 2, True, 1),
    (2, 16, 16, 192, 64, 3, 1, 2, False, 1),
]]
# (the reference on the first three images, as test_conv_c64_vs_fp32_reference_and_generic_kernel does: CPU time)
C64_CASES = [_case(600, 7, 33, 64, 64, 3, 1, 1, False, 0, 3), _case(6, 100, 210, 64, 64, 3, 1, 1, True, 0, 3)]
S2_CASES = [_case(*c) for c in [
    (5, 14, 14, 256, 256, 3, 2, 0, False, 0),
    (3, 28, 28, 64, 128, 3, 2, 1, False, 0),
    (3, 30, 22, 128, 256, 3, 2, 1, False, 0),
]]
WINO_CASES = [_case(*c) for c in [
    (3, 14, 14, 256, 256, 3, 1, 2, False, 1),
    (1, 2, 2, 64, 128, 3, 1, 0, False, 1),
    (7, 6, 30, 192, 160, 3, 1, 2, True, 1),
    (33, 4, 4, 128, 128, 3, 1, 1, True, 0),
    (1, 16, 16, 64, 64, 3, 1, 0, False, 0),
    (4, 136, 240, 128, 128, 3, 1, 1, False, 0, 1),      # the 2-D tiles; reference on the first image
]]
# F8_CASES rows 2 and 5: the fp16 outputs of the fp8 kernel (unit scales; the E4M3 codes of the same small integers)
F8_CASES = [_case(3, 14, 14, 256, 256, 3, 1, 0, True, 0), _case(1, 5, 9, 128, 96, 3, 1, 1, False, 0)]

ALL_CASES = list(dict.fromkeys(GENERIC_CASES + LEAN_CASES + C64_CASES + S2_CASES + WINO_CASES + F8_CASES))
ROUNDING_BIAS = (2049.0, 3000.5, 5001.0, -4097.0, 65000.0, -65510.0, 0.5, -1.5)
PLANT = 400     # receptive-field entries matched to one weight row (below): a sum of +800 / -800 at one pixel; a smaller field whole


def case_id(c):
    return "x".join(str(int(v)) for v in c[:10])


def out_dims(c):
    pad = c.k // 2
    return (c.H + 2 * pad - c.k) // c.stride + 1, (c.W + 2 * pad - c.k) // c.stride + 1


def border_classes(Ho, Wo):
    cy = np.where(np.arange(Ho) == 0, 0, np.where(np.arange(Ho) == Ho - 1, 2, 1))
    cx = np.where(np.arange(Wo) == 0, 0, np.where(np.arange(Wo) == Wo - 1, 2, 1))
    return cy[:, None] * 3 + cx[None, :]


def _plant_field(c):
    """the output pixel (n, oy, ox) at the centre of the last image and the in-image entries (iy, ix, kh, kw) of its receptive field"""
    Ho, Wo = out_dims(c)
    oy, ox, pad = Ho // 2, Wo // 2, c.k // 2
    taps = [(oy * c.stride - pad + kh, ox * c.stride - pad + kw, kh, kw) for kh in range(c.k) for kw in range(c.k)]
    return (c.N - 1 if c.ref_images == c.N else 0, oy, ox), [t for t in taps if 0 <= t[0] < c.H and 0 <= t[1] < c.W]


def rounding_expectations(c):
    """Which of the rounding set's events the issue's data CAN produce for a case - arithmetic, not observation:
    ties need an fp16 output; +inf needs 65000 + sum >= 65520, i.e. a sum of 520, which the PLANT matched entries (2 each)
    reach only where the field has that many.  -inf needs -65510 + sum + residual <= -65520, a sum of -10 - 16 at the most: the
    smallest field here has 64 entries, and matched whole it sums to -128, so EVERY case reaches it - where it survives the
    activation: ReLU clamps it to 0 and a PReLU slope of at most 0.5 halves it back into range."""
    fp16 = not (c.flags & OUT_F32)
    planted = len(_plant_field(c)[1]) * c.Cin >= PLANT
    return dict(ties=fp16, pos_inf=fp16 and planted, neg_inf=fp16 and c.act == 0)


def _ro(a):
    if a is not None:
        a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=6)
def exact_operands(case, seed=0, kind="exact"):
    """Operands of `case` and the float64 reference of the epilogue in the kernels' order: conv, bias (or 9-class border bias),
    residual (2x upsampled with flag bit 2), activation, ONE rounding to the output type.  kind "exact": every final value is
    representable, the rounding is the identity; kind "rounding": the same x, w and residual with the per-cout bias cycling
    through ROUNDING_BIAS (one step further per border class), so that the one rounding meets ties and both overflows.
    x in {-2..2} and w in {-1, 0, 1} lean to the positive side: 2049 + sum is odd, hence a tie of the 2-spaced [2048, 4096], for
    every even sum >= 0, and -4097 + sum is one for the even sums > 0 that bring it inside (-4096, -2048].  At the centre pixel of
    one image PLANT field entries - the whole field where it has fewer - are matched to the weights of the two couts whose bias
    is 65000 / -65510 there: sums of +800 and -800 (+-2 per entry of a smaller field), the overflows of the rounding set.
    -> dict of read-only arrays: x w bias slope res, ref (float64, the first ref_images images), ref_out (rounded), sum_abs."""
    c = case
    rng = np.random.default_rng([seed, *[int(v) for v in c[:10]]])
    Ho, Wo = out_dims(c)
    x = rng.choice(np.arange(-2, 3), size=(c.N, c.H, c.W, c.Cin), p=[0.1, 0.15, 0.2, 0.25, 0.3]).astype(np.float16)
    w = rng.choice(np.arange(-1, 2), size=(c.Cout, c.k, c.k, c.Cin), p=[0.2, 0.3, 0.5]).astype(np.float16)
    cls = border_classes(Ho, Wo) if c.flags & BORDER else np.zeros((Ho, Wo), int)
    (pn, py, px), field = _plant_field(c)
    shift = int(cls[py, px])
    co_pos, co_neg = (4 - shift) % 8, (5 - shift) % 8              # bias 65000 / -65510 at that pixel in the rounding set
    left = PLANT
    for (iy, ix, kh, kw) in field:
        n = min(left, c.Cin)
        if n <= 0:
            break
        sign = rng.choice(np.array([-1, 1]), size=n).astype(np.float16)
        w[co_pos, kh, kw, :n] = sign
        w[co_neg, kh, kw, :n] = -sign
        x[pn, iy, ix, :n] = 2 * sign
        left -= n
    bias = rng.integers(-8, 9, size=(9, c.Cout) if c.flags & BORDER else (c.Cout,)).astype(np.float32)
    if kind != "exact":                                          # (drawn all the same: slopes and residual are those of the exact set)
        cyc = np.array(ROUNDING_BIAS, np.float32)
        rows = [cyc[(np.arange(c.Cout) + k) % 8] for k in range(9)]
        bias = np.stack(rows) if c.flags & BORDER else rows[0]
    slope = rng.choice(np.array([0.5, 0.25], np.float32), size=c.Cout) if c.act == 2 else None
    res = None
    if c.res:
        res = rng.integers(-16, 17, size=(c.N, Ho // 2, Wo // 2, c.Cout) if c.flags & RES_UP2 else (c.N, Ho, Wo, c.Cout)).astype(np.float16)
    sub = slice(0, c.ref_images)
    xt = torch.from_numpy(x[sub].astype(np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2)
    y = F.conv2d(xt, wt, None, stride=c.stride, padding=c.k // 2).permute(0, 2, 3, 1).numpy()
    # condition (a): sum |x w| over a receptive field (integers far below 2^24: this sum itself is exact in fp32)
    sum_abs = float(F.conv2d(xt.abs().float(), wt.abs().float(), None, stride=c.stride, padding=c.k // 2).max())
    y = y + (bias.astype(np.float64)[cls][None] if c.flags & BORDER else bias.astype(np.float64))
    if res is not None:
        r = res[sub].astype(np.float64)
        y = y + (np.repeat(np.repeat(r, 2, axis=1), 2, axis=2) if c.flags & RES_UP2 else r)
    if c.act == 1:
        y = np.maximum(y, 0)
    elif c.act == 2:
        y = np.where(y > 0, y, y * slope.astype(np.float64))
    with np.errstate(over="ignore"):
        ref_out = y.astype(np.float32 if c.flags & OUT_F32 else np.float16)       # numpy: round to nearest even, once
    return {k: _ro(v) for k, v in dict(x=x, w=w, bias=bias, slope=slope, res=res, ref=y, ref_out=ref_out).items()} | dict(sum_abs=sum_abs)


def tie_mask(ref, ref16):
    """elements of the float64 `ref` that lie exactly halfway between two fp16 values (ref16 = its rounding)"""
    fin = np.isfinite(ref16)
    r = np.where(fin, ref16, np.float16(0))
    with np.errstate(over="ignore"):                    # (a step beyond 65504 is inf: excluded below)
        toward = np.nextafter(r, np.where(ref > r.astype(np.float64), np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    d0, d1 = np.abs(ref - r.astype(np.float64)), np.abs(ref - toward.astype(np.float64))
    return fin & np.isfinite(toward) & (d0 > 0) & (d0 == d1)


def winograd_operands(x, w):
    """F(2,3) along the rows in float64: V = B^T d per pixel pair (d0 - d2, d1 + d2, d2 - d1, d1 - d3 of columns 2p - 1 .. 2p + 2,
    zero beyond the row) [4][N, Cin, H, W / 2] and U = G g (g0, (g0 + g1 + g2) / 2, (g0 - g1 + g2) / 2, g2) [4][Cout, Cin, 3]"""
    xp = np.pad(x.astype(np.float64).transpose(0, 3, 1, 2), ((0, 0), (0, 0), (0, 0), (1, 1)))
    P = x.shape[2] // 2
    d = [xp[..., j::2][..., :P] for j in range(4)]
    V = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    g = [w.astype(np.float64)[:, :, kw, :].transpose(0, 2, 1) for kw in range(3)]          # [Cout, Cin, kh]
    U = [g[0], (g[0] + g[1] + g[2]) / 2, (g[0] - g[1] + g[2]) / 2, g[2]]
    return V, U


def winograd_sum_abs(V, U):
    """largest sum |V U| over (kernel row, channel) of any frequency, pixel pair and cout"""
    worst = 0.0
    for f in range(4):
        s = F.conv2d(torch.from_numpy(np.abs(V[f])).float(), torch.from_numpy(np.abs(U[f])).float()[..., None], None, padding=(1, 0))
        worst = max(worst, float(s.max()))
    return worst


def is_fp16_exact(a):
    with np.errstate(over="ignore"):
        return bool(np.array_equal(a.astype(np.float16).astype(np.float64), a))


def footprint(poison, H, W, k=3, stride=1):
    """poison: bool [N, H, W] of input pixels -> bool [N, Ho, Wo]: the output pixels whose receptive field (zero padding, per
    image) holds one of them"""
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    pp = np.pad(poison, ((0, 0), (pad, pad), (pad, pad)))
    out = np.zeros((poison.shape[0], Ho, Wo), bool)
    for kh in range(k):
        for kw in range(k):
            out |= pp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride]
    return out


def poison_pixels(N, H, W):
    """about a dozen (n, y, x) where a leak would come from: the last row of image 1 and the first row of image 2, column 0 and
    column W - 1, the two pixels around the first 256-pixel tile seam, the first and the last pixel of the tensor"""
    seam = [divmod(m, H * W) for m in (255, 256)]
    pix = [(1, H - 1, 0), (1, H - 1, W // 2), (1, H - 1, W - 1), (2, 0, 0), (2, 0, W // 2), (2, 0, W - 1),
           (4, H // 2, 0), (4, H // 2, W - 1), (N - 2, 0, W - 1), (N - 2, H - 1, 0), (0, 0, 0), (N - 1, H - 1, W - 1)]
    pix += [(n, r // W, r % W) for n, r in seam if n < N]
    return sorted(set(pix))


# ---------------------------------------------------------------------------------------------------------------- device side

def _assert_bits(out, want, what):
    assert out.shape == want.shape and out.dtype == want.dtype, (out.shape, want.shape, out.dtype, want.dtype)
    u = np.uint32 if out.dtype == np.float32 else np.uint16
    bad = np.argwhere(out.view(u) != want.view(u))
    if len(bad):
        first = [tuple(int(i) for i in b) for b in bad[:4]]
        pytest.fail(f"{what}: {len(bad)} of {out.size} elements differ; first (n, y, x, c) {first}: got {[float(out[b]) for b in first]}"
                    f" want {[float(want[b]) for b in first]}")


def _run(engine, c, ops, route, x=None, res=None):
    return engine.conv2d(ops["x"] if x is None else x, ops["w"], ops["bias"], stride=c.stride, act=c.act, slope=ops["slope"],
                         res=ops["res"] if res is None else res, flags=c.flags | route)


def _check_exact(engine, c, route, kind):
    ops = exact_operands(c, 0, kind)
    assert ops["sum_abs"] < 2 ** 24
    if kind == "exact":
        assert np.array_equal(ops["ref_out"].astype(np.float64), ops["ref"])
    out = _run(engine, c, ops, route)
    _assert_bits(out[:c.ref_images], ops["ref_out"], f"{case_id(c)} route {route:#x} {kind}")


def _sets(cases):
    """(case, kind) of both operand sets; an fp32 output has nothing to round: exact set only"""
    return [pytest.param(c, k, id=f"{case_id(c)}-{k}") for c in cases for k in ("exact", "rounding") if k == "exact" or not (c.flags & OUT_F32)]


@pytest.mark.parametrize("tiles", [TILES_DEFAULT, TILES_QUARTER], ids=["default-tiles", "quarter-tiles"])
@pytest.mark.parametrize("case,kind", _sets(GENERIC_CASES))
def test_generic_kernel_returns_the_reference_bits(engine, case, tiles, kind):
    _check_exact(engine, case, GENERIC | tiles, kind)


@pytest.mark.parametrize("tiles", [TILES_DEFAULT, TILES_QUARTER], ids=["default-tiles", "quarter-tiles"])
@pytest.mark.parametrize("case,kind", _sets(LEAN_CASES))
def test_row_patch_kernel_returns_the_reference_bits(engine, case, tiles, kind):
    _check_exact(engine, case, NO_C64 | tiles, kind)


@pytest.mark.parametrize("route", [TILES_DEFAULT, TILES_DEFAULT | NO_C64], ids=["c64", "row-patch"])
@pytest.mark.parametrize("case,kind", _sets(C64_CASES))
def test_c64_kernel_returns_the_reference_bits(engine, case, route, kind):
    assert os.environ.get("FRP_C64_ALL") == "1"             # (tests/conftest.py: the ragged maps do run the 64 -> 64 kernel)
    _check_exact(engine, case, route, kind)


@pytest.mark.parametrize("case,kind", _sets(S2_CASES))
def test_stride2_row_patch_kernel_returns_the_reference_bits(engine, case, kind):
    """(against the generic kernel this one is held to 2 ulps, 90 % identical: another k order.  Exact data has no k order.)"""
    _check_exact(engine, case, S2 | TILES_DEFAULT, kind)


@pytest.mark.parametrize("case,kind", _sets(WINO_CASES))
def test_winograd_kernel_returns_the_reference_bits(engine, case, kind):
    ops = exact_operands(case, 0, kind)
    V, U = winograd_operands(ops["x"][:case.ref_images], ops["w"])
    assert all(is_fp16_exact(v) for v in V) and all(is_fp16_exact(u) for u in U)
    assert winograd_sum_abs(V, U) < 2 ** 23                 # (U holds multiples of 1/2: one bit less than for integers)
    _check_exact(engine, case, WINO, kind)


@pytest.mark.parametrize("case", F8_CASES, ids=case_id)
def test_fp8_kernel_returns_the_reference_bits(engine, case):
    """conv2d_f8 on the E4M3 codes of the same integers, unit scales, fp16 output (exact set only)"""
    from frp_amd import weights as wts
    c, ops = case, exact_operands(case, 0, "exact")
    assert ops["sum_abs"] < 2 ** 24 and np.array_equal(ops["ref_out"].astype(np.float64), ops["ref"])
    xq, wq = wts.fp8_e4m3_encode(ops["x"].astype(np.float32)), wts.fp8_e4m3_encode(ops["w"].astype(np.float32))
    assert np.array_equal(wts.FP8_E4M3[xq], ops["x"].astype(np.float32)) and np.array_equal(wts.FP8_E4M3[wq], ops["w"].astype(np.float32))
    out = engine.conv2d_f8(xq, wq, np.ones(c.Cout, np.float32), ops["bias"], act=c.act, slope=ops["slope"], res=ops["res"], flags=c.flags,
                           in_scale=1.0, out_scale=1.0)
    _assert_bits(out, ops["ref_out"], f"{case_id(c)} fp8")


# ---------------------------------------------------------------------------------------------------------------- impulse probes

IMPULSE_SHAPES = [(3, 20, 20, 64, 64), (2, 30, 33, 192, 256)]
# (stride-2 row-patch route: neither shape is eligible - it takes even maps and whole 128-cout tiles only -, and with bit 21 set an
# ineligible shape runs the generic kernel silently: no stride-2 probe rather than one that tests another kernel)
IMPULSE_ROUTES = {"generic": GENERIC | TILES_DEFAULT, "generic-quarter": GENERIC | TILES_QUARTER, "row-patch": NO_C64 | TILES_DEFAULT,
                  "winograd": WINO}


def impulse_positions(N, H, W):
    """[(copy, n, y, x)]: one copy of the N images per probe.  Corners of the first and the last image, the last pixel of image 0
    and the first of image 1, and - in the flattened pixel index of the WHOLE batch, which is what the tiles cut - the pixels
    255, 256, 511, 512 modulo 512: both sides of a 256- and of a 512-pixel tile seam.  The last corner of the last image goes
    into the last copy: the very last pixel of the batch, the end of the ragged last tile."""
    last = (N - 1, H - 1, W - 1)
    local = [(n, y, x) for n in (0, N - 1) for y in (0, H - 1) for x in (0, W - 1)] + [(0, H - 1, W - 1), (1, 0, 0)]
    local = [p for p in dict.fromkeys(local) if p != last]
    pos = [(j, *p) for j, p in enumerate(local)]
    for g in (255, 256, 511, 512):
        j = len(pos)
        m = (g - j * N * H * W) % 512
        pos.append((j, m // (H * W), (m % (H * W)) // W, m % W))
    pos.append((len(pos), *last))
    return pos


# (the Winograd kernel takes even widths only - test_conv_winograd_rejects_what_it_does_not_cover -: not the 33-wide shape)
IMPULSE_PROBES = [pytest.param(s, r, id="x".join(map(str, s)) + "-" + r) for s in IMPULSE_SHAPES for r in IMPULSE_ROUTES
                  if not (r == "winograd" and s[2] % 2)]


@pytest.mark.parametrize("shape,route", IMPULSE_PROBES)
def test_impulse_stamps(engine, shape, route):
    """A single 1 in channel c* under weights that carry the tap's code 1 + 3 kh + kw in that channel alone: the output is the
    flipped 3x3 stamp of the codes around the impulse, clipped at the image border, in every cout - and zero everywhere else."""
    N, H, W, Cin, Cout = shape
    pos = impulse_positions(N, H, W)
    want = np.zeros((len(pos) * N, H, W), np.float16)
    for (j, n, y, x) in pos:
        assert 0 <= n < N and 0 <= y < H and 0 <= x < W
        for kh in range(3):
            for kw in range(3):
                oy, ox = y + 1 - kh, x + 1 - kw
                if 0 <= oy < H and 0 <= ox < W:
                    want[j * N + n, oy, ox] = 1 + 3 * kh + kw
    want = np.ascontiguousarray(np.broadcast_to(want[..., None], want.shape + (Cout,)))
    for cstar in sorted({0, 63, Cin - 1}):
        xs = np.zeros((len(pos) * N, H, W, Cin), np.float16)
        for (j, n, y, x) in pos:
            xs[j * N + n, y, x, cstar] = 1
        w = np.zeros((Cout, 3, 3, Cin), np.float16)
        w[:, :, :, cstar] = (1 + np.arange(9, dtype=np.float16)).reshape(3, 3)
        out = engine.conv2d(xs, w, np.zeros(Cout, np.float32), flags=IMPULSE_ROUTES[route])
        _assert_bits(out, want, f"impulses in channel {cstar}, route {route}")


# ---------------------------------------------------------------------------------------------------------------- poison

# family -> (route, stride, shape (N, H, W, Cin, Cout), [(act, residual, flags)] for act none / PReLU, the ReLU configuration).
# The Winograd kernel does not take the 7-wide maps of the other direct families (even widths only): its case is the entry of
# WINO_CASES with many images per tile and a ragged last tile.  The stride-2 kernel has neither PReLU nor a residual, the 64 -> 64
# kernel exactly the four (activation, residual, border bias) combinations of the two networks.
POISON = {
    "generic": (GENERIC | TILES_DEFAULT, 1, (40, 7, 7, 128, 128), [(0, True, 0), (2, True, BORDER)], (1, True, 0)),
    "generic-quarter": (GENERIC | TILES_QUARTER, 1, (40, 7, 7, 128, 128), [(0, True, 0), (2, True, BORDER)], (1, True, 0)),
    "row-patch": (NO_C64 | TILES_DEFAULT, 1, (40, 7, 7, 128, 128), [(0, True, 0), (2, True, BORDER)], (1, True, 0)),
    "winograd": (WINO, 1, (33, 4, 4, 128, 128), [(0, True, 0), (2, True, BORDER)], (1, True, 0)),
    "stride2": (S2 | TILES_DEFAULT, 2, (5, 14, 14, 256, 256), [(0, False, 0)], (1, False, 0)),
    "c64": (TILES_DEFAULT, 1, (600, 7, 33, 64, 64), [(0, True, 0), (2, False, BORDER)], (1, True, 0)),
}


@functools.lru_cache(maxsize=2)
def _poison_operands(shape, stride):
    N, H, W, Cin, Cout = shape
    rng = np.random.default_rng([7, *shape, stride])
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float16)
    w = (rng.standard_normal((Cout, 3, 3, Cin)) / np.sqrt(9 * Cin)).astype(np.float16)
    bias = (rng.standard_normal((9, Cout)) * 0.3).astype(np.float32)
    slope = rng.uniform(0.1, 0.4, Cout).astype(np.float32)
    res = rng.standard_normal((N, H // stride, W // stride, Cout)).astype(np.float16)
    return tuple(_ro(a) for a in (x, w, bias, slope, res))


def _poison_setup(shape, stride, has_res):
    """-> x, w, bias9, slope, res, poisoned-pixel mask [N, H, W], element mask of the outputs that must be non-finite, residual
    elements to poison (pixels outside the footprint of the poisoned inputs)"""
    N, H, W, Cin, Cout = shape
    x, w, bias, slope, res = _poison_operands(shape, stride)
    pm = np.zeros((N, H, W), bool)
    for p in poison_pixels(N, H, W):
        pm[p] = True
    fp = footprint(pm, H, W, 3, stride)
    expect = np.ascontiguousarray(np.broadcast_to(fp[..., None], fp.shape + (Cout,)))
    relems = []
    if has_res:
        clear = np.argwhere(~fp)
        relems = [(*(int(v) for v in clear[len(clear) // 3]), 5), (*(int(v) for v in clear[-1]), Cout - 1)]
        for e in relems:
            expect[e] = True
    return x, w, bias, slope, res, pm, expect, relems


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("family", list(POISON))
def test_poisoned_pixels_reach_their_receptive_fields_only(engine, family, value):
    """NaN / +inf in a dozen input pixels (all channels) and in two residual elements: the non-finite outputs are exactly the 3x3
    dilation of the pixels (per image, zero padding; the stride-2 footprint for stride 2) in every cout plus the two residual
    elements' own outputs; every other element has the bits of the clean run of the same route."""
    route, stride, shape, configs, _ = POISON[family]
    if family == "c64":
        assert os.environ.get("FRP_C64_ALL") == "1"
    for (act, has_res, flags) in configs:
        x, w, bias, slope, res, pm, expect, relems = _poison_setup(shape, stride, has_res)
        kw = dict(stride=stride, act=act, slope=slope if act == 2 else None, flags=flags | route)
        b = bias if flags & BORDER else bias[0]
        clean = engine.conv2d(x, w, b, res=res if has_res else None, **kw)
        assert np.isfinite(clean).all()
        xp = x.copy()
        xp[pm] = value
        rp = None
        if has_res:
            rp = res.copy()
            for e in relems:
                rp[e] = value
        got = engine.conv2d(xp, w, b, res=rp, **kw)
        nonfinite = ~np.isfinite(got)
        wrong = np.argwhere(nonfinite != expect)
        assert len(wrong) == 0, (f"act {act}: {len(wrong)} elements are non-finite where they must be finite or the reverse; first "
                                 f"{wrong[:4].tolist()} got {[float(got[tuple(i)]) for i in wrong[:4]]}")
        _assert_bits(np.where(expect, np.float16(0), got), np.where(expect, np.float16(0), clean), f"{family} act {act} outside the footprint")


@pytest.mark.parametrize("family", list(POISON))
def test_poison_under_relu_matches_the_generic_kernel(engine, family):
    """ReLU on a non-finite sum ("What the conv epilogue guarantees"): outside the footprint the bits of the clean run,
    inside it the bits the generic kernel returns for the same poisoned operands - NaN inputs, one +inf residual element."""
    route, stride, shape, _, (act, has_res, flags) = POISON[family]
    x, w, bias, slope, res, pm, expect, relems = _poison_setup(shape, stride, has_res)
    kw = dict(stride=stride, act=act, flags=flags | route)
    clean = engine.conv2d(x, w, bias[0], res=res if has_res else None, **kw)
    xp = x.copy()
    xp[pm] = np.nan
    rp = None
    if has_res:
        rp = res.copy()
        rp[relems[0]] = np.inf
        rp[relems[1]] = np.nan
    got = engine.conv2d(xp, w, bias[0], res=rp, **kw)
    generic = engine.conv2d(xp, w, bias[0], res=rp, **(kw | dict(flags=flags | GENERIC | TILES_DEFAULT)))
    inside = got[expect]
    print(f"{family}: inside the footprint under ReLU: {np.unique(inside.view(np.uint16)).tolist()} (fp16 bit patterns)")
    _assert_bits(np.where(expect, np.float16(0), got), np.where(expect, np.float16(0), clean), f"{family} ReLU outside the footprint")
    _assert_bits(np.where(expect, got, np.float16(0)), np.where(expect, generic, np.float16(0)), f"{family} ReLU inside the footprint")
