"""The conditions tests/test_gpu_conv_exact.py rests on, asserted on its reference alone (no device): with these operands every
partial sum in any order is exact in fp32 and the exact set's results are representable in the output type, so a kernel that
differs from the reference in one bit is wrong; and the rounding set does meet ties and overflows."""
import numpy as np
import pytest

import test_gpu_conv_exact as gx


@pytest.mark.parametrize("case", gx.ALL_CASES, ids=gx.case_id)
def test_exact_set_is_exact(case):
    ops = gx.exact_operands(case, 0, "exact")
    x, w = ops["x"].astype(np.float64), ops["w"].astype(np.float64)
    assert set(np.unique(x)) <= {-2, -1, 0, 1, 2} and set(np.unique(w)) <= {-1, 0, 1}
    assert np.abs(ops["bias"]).max() <= 8 and np.array_equal(ops["bias"], np.round(ops["bias"]))
    assert ops["bias"].shape == ((9, case.Cout) if case.flags & gx.BORDER else (case.Cout,))
    if ops["res"] is not None:
        assert np.abs(ops["res"].astype(np.float64)).max() <= 16
    if ops["slope"] is not None:
        assert set(np.unique(ops["slope"])) <= {0.5, 0.25}
    # (a) every partial sum in any order is an integer below 2^24: exact in fp32
    assert ops["sum_abs"] < 2 ** 24
    # (b) the one rounding to the output type is the identity
    assert ops["ref"].shape[0] == case.ref_images
    assert np.array_equal(ops["ref_out"].astype(np.float64), ops["ref"])
    assert ops["ref_out"].dtype == (np.float32 if case.flags & gx.OUT_F32 else np.float16)


@pytest.mark.parametrize("case", gx.WINO_CASES, ids=gx.case_id)
def test_winograd_transforms_of_the_exact_set_are_exact(case):
    """(a) for the Winograd kernel: its fp16 operands are the F(2,3) transforms; both are representable, their sums exact"""
    ops = gx.exact_operands(case, 0, "exact")
    V, U = gx.winograd_operands(ops["x"][:case.ref_images], ops["w"])
    assert all(gx.is_fp16_exact(v) for v in V) and all(gx.is_fp16_exact(u) for u in U)
    assert max(np.abs(v).max() for v in V) <= 4 and max(np.abs(u).max() for u in U) <= 1.5
    assert gx.winograd_sum_abs(V, U) < 2 ** 23                # multiples of 1/2 (U): every partial sum exact in fp32 below 2^23
    # ... and they are the transforms of this convolution: the output pair (M0 + M1 + M2, M1 - M2 - M3) is the reference's
    n, y, co = 0, case.H // 2, 3
    M = [sum(V[f][n, :, y + kh - 1, :].T @ U[f][co, :, kh] for kh in range(3) if 0 <= y + kh - 1 < case.H) for f in range(4)]
    pair = np.stack([M[0] + M[1] + M[2], M[1] - M[2] - M[3]], axis=1).reshape(-1)
    xt, wt = ops["x"][n].astype(np.float64), ops["w"][co].astype(np.float64)
    xp = np.pad(xt, ((1, 1), (1, 1), (0, 0)))
    direct = np.array([(xp[y:y + 3, ox:ox + 3] * wt).sum() for ox in range(case.W)])
    assert np.array_equal(pair, direct)


@pytest.mark.parametrize("case", [c for c in gx.ALL_CASES if c not in gx.F8_CASES and not (c.flags & gx.OUT_F32)], ids=gx.case_id)
def test_rounding_set_meets_ties_and_overflows(case):
    """Shares of the rounding set, on the reference alone.  At least 10 % of the outputs are exact ties; under ReLU three of the
    eight bias classes (-4097, -65510, -1.5) end at 0 and 3000.5 never ties, which caps the share of the whole tensor at
    (1/2 + 1/4 + 1/32) / 8 < 10 %, so there the share is taken of the outputs the ReLU leaves to the rounding (reference > 0).
    -inf: in every case whose outputs can hold it (fp16, no activation: ReLU and PReLU bring -65510 + sum back into range).
    +inf: wherever the field has the 400 entries a sum of 520 needs (gx.rounding_expectations)."""
    exact, ops = gx.exact_operands(case, 0, "exact"), gx.exact_operands(case, 0, "rounding")
    for k in ("x", "w", "res", "slope"):
        assert (ops[k] is None and exact[k] is None) or np.array_equal(ops[k], exact[k])
    assert ops["sum_abs"] < 2 ** 24
    bias = ops["bias"] if case.flags & gx.BORDER else ops["bias"][None]
    for k, row in enumerate(bias):
        assert np.array_equal(row, np.array(gx.ROUNDING_BIAS, np.float32)[(np.arange(case.Cout) + k) % 8])
    ref, out = ops["ref"], ops["ref_out"]
    ties = gx.tie_mask(ref, out)
    pool = ref > 0 if case.act == 1 else np.ones(ref.shape, bool)
    share = ties[pool].mean()
    print(f"{gx.case_id(case)}: ties {share:.3f} of {int(pool.sum())}, +inf {int(np.isposinf(out).sum())}, -inf {int(np.isneginf(out).sum())}")
    assert share >= 0.10
    # the ties round to even: numpy's cast is the round-to-nearest-even the kernels' one conversion has to be
    assert np.all((out[ties].view(np.uint16) & 1) == 0)
    want = gx.rounding_expectations(case)
    if want["pos_inf"]:
        assert np.isposinf(out).any()
    assert want["neg_inf"] == (case.act == 0)
    if want["neg_inf"]:
        assert np.isneginf(out).any()
    assert np.isnan(out).sum() == 0


def test_rounding_set_overflows_in_every_family():
    for fam in (gx.GENERIC_CASES, gx.LEAN_CASES, gx.S2_CASES, gx.WINO_CASES):
        assert any(gx.rounding_expectations(c)["pos_inf"] for c in fam) and any(gx.rounding_expectations(c)["neg_inf"] for c in fam)
    assert all(gx.rounding_expectations(c)["pos_inf"] for c in gx.C64_CASES)      # (both 64 -> 64 cases are ReLU layers: no -inf)


def test_tie_mask_on_known_values():
    ref = np.array([2049.0, 2050.0, 2051.0, 3000.5, 4098.0, 0.5, 65520.0, 65519.0, -2049.0, 1024.5, 2048.0 + 2 ** -20])
    with np.errstate(over="ignore"):
        got = gx.tie_mask(ref, ref.astype(np.float16))
    assert got.tolist() == [True, False, True, False, True, False, False, False, True, True, False]


def test_footprint_against_a_brute_force_loop():
    rng = np.random.default_rng(5)
    poison = rng.random((2, 5, 5)) < 0.12
    poison[0, 4, 4] = poison[1, 0, 0] = True                 # the last pixel of image 0 and the first of image 1
    for stride, size in ((1, 5), (2, 6)):
        p = np.zeros((2, size, size), bool)
        p[:, :5, :5] = poison
        Ho = (size + 2 - 3) // stride + 1
        want = np.zeros((2, Ho, Ho), bool)
        for n in range(2):
            for oy in range(Ho):
                for ox in range(Ho):
                    for kh in range(3):
                        for kw in range(3):
                            iy, ix = oy * stride - 1 + kh, ox * stride - 1 + kw
                            if 0 <= iy < size and 0 <= ix < size and p[n, iy, ix]:
                                want[n, oy, ox] = True
        assert np.array_equal(gx.footprint(p, size, size, 3, stride), want)
        assert not want[1, Ho - 1, Ho - 1] or p[1, size - 3:, size - 3:].any()
    # nothing crosses from one image into the next
    one = np.zeros((2, 5, 5), bool)
    one[0, 4, 4] = True
    assert not gx.footprint(one, 5, 5)[1].any() and gx.footprint(one, 5, 5)[0].sum() == 4


def test_poison_and_impulse_positions_are_where_the_issue_wants_them():
    for (route, stride, shape, configs, relu) in gx.POISON.values():
        N, H, W = shape[:3]
        pix = gx.poison_pixels(N, H, W)
        assert 10 <= len(pix) <= 16 and all(0 <= n < N and 0 <= y < H and 0 <= x < W for n, y, x in pix)
        assert (N - 1, H - 1, W - 1) in pix and any(y == H - 1 for _, y, _ in pix) and any(y == 0 for _, y, _ in pix)
        assert any(x == 0 for _, _, x in pix) and any(x == W - 1 for _, _, x in pix)
        assert N * (H // stride) * (W // stride) % 256 != 0 and (stride == 2 or N * H * W > 256)      # a ragged last tile; several tiles
    for (N, H, W, Cin, Cout) in gx.IMPULSE_SHAPES:
        pos = gx.impulse_positions(N, H, W)
        flat = [((j * N + n) * H + y) * W + x for j, n, y, x in pos[-5:-1]]
        assert [m % 512 for m in flat] == [255, 256, 511, 0]
        assert len({j for j, *_ in pos}) == len(pos)
        corners = {(n, y, x) for n in (0, N - 1) for y in (0, H - 1) for x in (0, W - 1)}
        assert {p[1:] for p in pos[:-5]} | {pos[-1][1:]} == corners | {(0, H - 1, W - 1), (1, 0, 0)}
        j, n, y, x = pos[-1]
        assert ((j * N + n) * H + y) * W + x == len(pos) * N * H * W - 1          # the last pixel of the batch
        assert (len(pos) * N * H * W) % 256 != 0                                 # ... in a ragged last tile
