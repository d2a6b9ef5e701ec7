"""CPU tests of the quality gate's host model (frp_amd/quality_gate.py): against FaceService.quality_from_sums and box_to_location,
the correctly rounded quotient against fractions.Fraction, and the gate of a whole pass (validity, the two bounds, the frame-major
face list) against the reference's own assessment."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import quality_model
from fake_engine import FakeEngine
from frp_amd import quality_gate as qg
from frp_amd.face_service import FaceService, box_to_location

QUALITY_KEYS = ["score", "size_score", "position_score", "aspect_score", "blur_score", "lighting_score", "issues"]
N4K = 3840 * 2160
SUMS_4K = [N4K // 2 * 255, N4K // 2 * 65025, 0, N4K * 2040 * 2040]      # the 4K checkerboard of tests/test_quality_host.py


def _cases():
    """(name, RGB image, location): the cases of tests/test_quality_host.py::_cases"""
    rng = np.random.default_rng(20240607)
    out = []
    noise = rng.integers(0, 256, size=(240, 320, 3), dtype=np.uint8)
    for loc in ((0, 320, 240, 0), (17, 131, 90, 40), (100, 101, 240, 3), (239, 320, 240, 250)):
        out.append((f"noise{loc}", noise, loc))
    smooth = np.clip(128 + 40 * np.sin(np.arange(320) / 9.0)[None, :, None] + rng.normal(0, 3, size=(240, 320, 3)), 0, 255).astype(np.uint8)
    out.append(("smooth", smooth, (20, 300, 200, 30)))
    dark = rng.integers(0, 40, size=(97, 131, 3), dtype=np.uint8)
    out.append(("dark", dark, (3, 131, 97, 1)))
    yy, xx = np.mgrid[0:64, 0:64]
    cb = np.stack([(((yy + xx) % 2) * 255).astype(np.uint8)] * 3, -1)
    out.append(("checkerboard", cb, (0, 64, 64, 0)))
    out.append(("flat", np.full((64, 64, 3), 128, np.uint8), (0, 64, 64, 0)))
    out.append(("1x1", noise, (5, 8, 6, 7)))
    out.append(("1x17", noise, (9, 30, 10, 13)))
    out.append(("17x1", noise, (9, 14, 26, 13)))
    return out


def _bits(v):
    return struct.unpack("<q", struct.pack("<d", float(v)))[0]


def test_model_equals_quality_from_sums():
    """rounded dicts equal; unrounded blur / lighting bit-equal (no pow in them); unrounded overall within 1e-12 - at most a dozen
    float64 operations on values <= 128 differ by at most one ulp each (2.8e-14), so the sum stays below 3.4e-13"""
    fs = FaceService(engine=FakeEngine())
    for name, img, loc in _cases():
        top, right, bottom, left = loc
        s = quality_model.sums(img[None], (0, top, right, bottom, left), rgb=True)
        want = fs.quality_from_sums(img.shape, loc, (bottom - top) * (right - left), s)
        hist = fs._quality_history[-1]
        H, W = img.shape[:2]
        assert np.array_equal(qg.crop_sums(img[None], 0, loc, rgb=True), s), name
        sc = qg.scores_from_sums(H, W, loc, s)
        got = qg.quality_dict(loc, sc)
        assert list(got.keys()) == QUALITY_KEYS
        assert got == want, (name, got, want)
        assert _bits(sc[4]) == _bits(hist["blur_score"]) and _bits(sc[5]) == _bits(hist["lighting_score"]), name
        assert abs(sc[0] - hist["score"]) <= 1e-12, (name, sc[0], hist["score"])
    # the empty crop: the reference's except branch
    empty = qg.scores_from_sums(240, 320, (10, 5, 30, 5), None)
    assert empty[4] == 50.0 and empty[5] == 50.0
    assert qg.quality_dict((10, 5, 30, 5), empty) == fs.assess_face_quality(np.zeros((240, 320, 3), np.uint8), (10, 5, 30, 5))


def test_gate_location_is_box_to_location_on_finite_boxes():
    rng = np.random.default_rng(3)
    H, W = 97, 131
    boxes = [rng.uniform(-300, 300, 4) for _ in range(300)] + [rng.uniform(-2.0 ** 30, 2.0 ** 30, 4) * 0.999 for _ in range(100)]
    boxes += [[-0.5, -0.99, 0.99, 0.5], [10.7, 20.2, 110.9, 140.1], [-5.0, 3.0, 700.0, 500.0], [130.999, 96.999, 131.0, 97.0],
              [2.0 ** 30 - 64, -(2.0 ** 30 - 64), 5.5, 7.25], [0, 0, 0, 0]]
    for b in boxes:
        b32 = np.asarray(b, np.float32)
        assert all(abs(float(v)) < 2.0 ** 30 for v in b32)
        assert qg.gate_location(b32, H, W) == box_to_location(b32, H, W), b
    # beyond the limit the clamp decides; a non-finite coordinate makes the face invalid
    assert qg.gate_location([-3e38, -1e10, 3e38, 1e10], H, W) == (0, W, H, 0)
    assert qg.gate_location([3e38, 1e10, -3e38, -1e10], H, W) == (2 ** 30, -2 ** 30, -2 ** 30, 2 ** 30)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for i in range(4):
            b = [1.0, 2.0, 30.0, 40.0]
            b[i] = bad
            assert qg.gate_location(b, H, W) is None


def _assert_correctly_rounded(got: float, exact: Fraction):
    err = abs(Fraction(got) - exact)
    for nb in (math.nextafter(got, math.inf), math.nextafter(got, -math.inf)):
        e = abs(Fraction(nb) - exact)
        assert err < e or (err == e and _bits(got) % 2 == 0), (got, nb)


def test_quotient_is_correctly_rounded_beyond_2_63():
    s1, s2, l1, l2 = SUMS_4K
    assert N4K * l2 > 2 ** 63
    _assert_correctly_rounded(qg.variance(N4K, l1, l2), Fraction(N4K * l2 - l1 * l1, N4K * N4K))
    _assert_correctly_rounded(qg.variance(N4K, s1, s2), Fraction(N4K * s2 - s1 * s1, N4K * N4K))
    rng = np.random.default_rng(11)
    for _ in range(200):                      # quotients that are not representable: odd numerators over the same denominator
        n = int(rng.integers(2, N4K))
        l2 = int(rng.integers(0, n * 1040400))
        l1 = int(rng.integers(0, math.isqrt(n * l2) + 1))
        _assert_correctly_rounded(qg.variance(n, l1, l2), Fraction(n * l2 - l1 * l1, n * n))
    sc = qg.scores_from_sums(2160, 3840, (0, 3840, 2160, 0), SUMS_4K)
    assert sc[4] == 100.0 and round(sc[5], 2) == round((100.0 - 0.5 / 128 * 100 + 100.0) / 2, 2)


# ------------------------------------------------------------------ the gate of a whole pass
H, W, K = 240, 320, 4
NAN = float("nan")
BOXES = [[[10.7, 20.2, 110.9, 140.1], [-5.0, 3.0, 400.0, 300.0], [300.0, 10.0, 312.0, 19.0], [0, 0, 0, 0]],
         [[NAN, 1.0, 20.0, 20.0], [400.0, 10.0, 460.0, 50.0], [30.5, 40.5, 130.5, 150.5], [5.0, 5.0, 6.0, 6.0]],
         [[1.0, 1.0, 50.0, 50.0]] * 4]


def test_gate_of_a_pass():
    frames = np.random.default_rng(9).integers(0, 256, size=(3, H, W, 3), dtype=np.uint8)
    boxes = np.array(BOXES, np.float32)
    ref = FaceService(engine=FakeEngine())
    counts = (3, K + 3, -1)                     # clamped to 3, K, 0
    g = qg.gate(frames, boxes, counts)
    assert g["scores"].shape == (3, K, 8) and g["scores"].dtype == np.float64 and g["sums"].dtype == np.int64
    # slots at or beyond the count are zero
    for name in ("scores", "passed", "rects", "sums"):
        assert not g[name][0, 3].any() and not g[name][2].any(), name
    # an invalid face: -1.0 and zeros, never passes; an empty crop: the reference's default blur / lighting, and it is valid
    assert g["scores"][1, 0].tolist() == list(qg.INVALID_SCORES) and g["passed"][1, 0] == 0 and not g["rects"][1, 0].any()
    assert g["rects"][1, 1].tolist() == [10, 320, 50, 400] and g["scores"][1, 1, 4] == 50.0 and g["scores"][1, 1, 5] == 50.0
    assert g["passed"][1, 1] == 1
    # 0 / 0 passes every valid face; the list is frame-major
    assert g["passed"].tolist() == [[1, 1, 1, 0], [0, 1, 1, 1], [0, 0, 0, 0]] and g["n_embed"] == 6
    assert g["face_slot"].tolist() == [0, 1, 2, K + 1, K + 2, K + 3] + [-1] * (3 * K - 6)
    # the dicts are the reference's (BGR frames, as the camera loop delivers them), sums those of the tests' integer model
    for b, k in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (1, 3)):
        loc = tuple(int(v) for v in g["rects"][b, k])
        assert loc == box_to_location(boxes[b, k], H, W)
        assert qg.quality_dict(loc, g["scores"][b, k]) == ref.assess_face_quality(frames[b][..., ::-1], loc), (b, k)
        if not qg.is_empty(loc):
            assert np.array_equal(g["sums"][b, k], quality_model.sums(frames, (b,) + loc))
    assert not np.array_equal(qg.gate(frames, boxes, counts, rgb=True)["sums"], g["sums"])
    # the bounds, on unrounded values: a score between two faces' scores, the shorter side, both
    live = g["scores"][..., 0][g["passed"] == 1]
    s = np.sort(live)
    mid = float((s[2] + s[3]) / 2)
    assert s[3] - s[2] > 1e-6
    by_score = qg.gate(frames, boxes, counts, mid, 0)
    assert np.array_equal(by_score["passed"] == 1, (g["passed"] == 1) & (g["scores"][..., 0] >= mid)) and by_score["n_embed"] == 3
    assert np.array_equal(by_score["scores"], g["scores"])
    by_side = qg.gate(frames, boxes, counts, 0.0, 10)
    assert by_side["passed"].tolist() == [[1, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]       # 12 x 9, the empty crop and 1 x 1 are out
    assert by_side["face_slot"][:3].tolist() == [0, 1, K + 2] and by_side["n_embed"] == 3
    assert qg.gate(frames, boxes, counts, 101.0, 0)["n_embed"] == 0
    exact = float(g["scores"][0, 0, 0])           # a bound equal to a score passes it; the next double does not
    assert qg.gate(frames, boxes, counts, exact, 0)["passed"][0, 0] == 1
    assert qg.gate(frames, boxes, counts, math.nextafter(exact, math.inf), 0)["passed"][0, 0] == 0
    for bad in ((-1.0, 0), (NAN, 0), (float("inf"), 0), (10.0, -1), (10.0, 1.5)):
        with pytest.raises(ValueError):
            qg.gate(frames, boxes, counts, *bad)
