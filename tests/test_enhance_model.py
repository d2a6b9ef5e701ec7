"""CPU tests of the enhancer's integer model (tests/enhance_model.py) against Pillow itself: resize(BICUBIC), GaussianBlur and
UnsharpMask, byte for byte; the inputs' reach (what the device tests rely on them to exercise); enhanced_size against the values
the reference's _safe_resize_params gave (tests/golden/enhance_sizes.json)."""
import json
import os

import numpy as np
import pytest
from PIL import Image, ImageFilter

import enhance_model as M
from enhance_cases import DEFAULT, PARAMS, SIZES, content
from frp_amd import face_service

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("noise", "ramp")


def _same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8, (what, a.shape, b.shape)
    bad = np.argwhere(a != b)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(SIZES))
def test_resample_equals_pillow(name, kind):
    w, h, ow, oh = SIZES[name]
    img = content(kind, h, w, seed=1)
    got = M.resample(img, ow, oh)
    want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
    _same(got, want, name)
    for n_in, n_out in ((w, ow), (h, oh)):
        if n_out != n_in:
            assert max(len(k) for _, k in M.taps(n_in, n_out)) <= M.MAX_TAPS


@pytest.mark.parametrize("radius", [0.0, 0.5, 1.0, 1.5, 2.0])
@pytest.mark.parametrize("kind", KINDS)
def test_gaussian_blur_equals_pillow(kind, radius):
    for name in ("a_1x1", "b_3x5", "c_x2"):
        w, h, _, _ = SIZES[name]
        img = content(kind, h, w, seed=2)
        _same(M.gaussian_blur(img, radius), np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(radius))), (name, radius))


def test_box_weights_of_the_default_radius():
    """radius 1: a 3-tap filter, six times; the weight is a FLOAT quotient (2^24 / 1.5 rounds up to ...811)"""
    assert M.box_params(1.0) == (0, 11184811, 2796202)
    assert M.box_params(0.0) == (0, 1 << 24, 0)
    assert M.box_params(2.0)[0] == 1 and M.box_params(0.5)[0] == 0


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(SIZES))
def test_enhance_equals_pillow(name, kind, params):
    w, h, ow, oh = SIZES[name]
    radius, percent, threshold, sharpen = params
    img = content(kind, h, w, seed=3)
    got = M.enhance(img, ow, oh, radius, percent, threshold, sharpen)
    _same(got, M.pillow_enhance(img, ow, oh, radius, percent, threshold, sharpen), (name, kind, params))
    if sharpen:
        res = M.resample(img, ow, oh)
        pil = np.asarray(Image.fromarray(res).filter(ImageFilter.UnsharpMask(radius=radius, percent=percent, threshold=threshold)))
        _same(M.unsharp(res, radius, percent, threshold), pil, ("unsharp alone", name, kind, params))


def test_inputs_reach_the_threshold_the_division_and_both_clips():
    """on the model's own intermediates, for the default parameters over the cases' inputs: a device error at any of these
    places cannot hide behind inputs that never get there"""
    radius, percent, threshold, _ = DEFAULT
    seen = dict.fromkeys(("at_threshold", "above_threshold", "negative_inexact", "clip_0", "clip_255"), 0)
    per_kind = {k: 0 for k in KINDS}
    for name, (w, h, ow, oh) in SIZES.items():
        for kind in KINDS:
            res = M.resample(content(kind, h, w, seed=3), ow, oh)
            _, d, unclipped = M.unsharp_parts(res, radius, percent, threshold)
            active = np.abs(d) > threshold
            seen["at_threshold"] += int((np.abs(d) == threshold).sum())
            seen["above_threshold"] += int((np.abs(d) == threshold + 1).sum())
            seen["negative_inexact"] += int(((d < 0) & active & ((d * percent) % 100 != 0)).sum())
            seen["clip_0"] += int((active & (unclipped < 0)).sum())
            seen["clip_255"] += int((active & (unclipped > 255)).sum())
            per_kind[kind] += int((np.abs(d) == threshold).sum()) + int((np.abs(d) == threshold + 1).sum())
    print(seen, per_kind)
    assert all(v > 0 for v in seen.values()), seen
    assert per_kind["ramp"] > 0 and per_kind["noise"] > 0, per_kind      # both sides of the threshold, in both kinds of input


def test_division_truncates_toward_zero():
    img = np.zeros((5, 5, 3), np.uint8) + 100
    img[2, 2] = 60                                       # darker than its blur: d < 0 there, > 0 around it
    out, d, unclipped = M.unsharp_parts(img, 1.0, 120, 0)
    assert d[2, 2, 0] < 0 and (d[2, 2, 0] * 120) % 100 != 0
    assert unclipped[2, 2, 0] == 60 - ((-d[2, 2, 0] * 120) // 100)
    _same(out, np.asarray(Image.fromarray(img).filter(ImageFilter.UnsharpMask(radius=1.0, percent=120, threshold=0))), "dip")


def test_enhanced_size_equals_the_reference():
    rows = json.load(open(os.path.join(HERE, "golden", "enhance_sizes.json")))
    asked = {(r["w"], r["h"], r["upscale"]) for r in rows}
    assert {(1920, 1080, 2.0), (3840, 2160, 2.0), (97561, 41, 2.0), (5, 3, 1.5)} <= asked        # the .5 case: 7.5 -> 8, 4.5 -> 4
    for r in rows:
        want = (r["new_w"], r["new_h"])
        assert M.enhanced_size(r["w"], r["h"], r["upscale"], r["max_pixels"]) == want, r
        assert face_service.enhanced_size(r["w"], r["h"], r["upscale"], r["max_pixels"]) == want, r
    assert M.enhanced_size(1920, 1080) == (2667, 1500)


def test_enhancer_settings_follow_the_reference(monkeypatch):
    for k in ("ENHANCER_UPSCALE_FACTOR", "ENHANCER_MAX_PIXELS", "ENHANCER_JPEG_QUALITY", "ENHANCER_SHARPEN"):
        monkeypatch.delenv(k, raising=False)
    assert face_service.enhancer_settings() == (2.0, 4_000_000, 85, True)
    monkeypatch.setenv("ENHANCER_UPSCALE_FACTOR", "1.5")
    monkeypatch.setenv("ENHANCER_MAX_PIXELS", "1000")
    monkeypatch.setenv("ENHANCER_JPEG_QUALITY", "70")
    monkeypatch.setenv("ENHANCER_SHARPEN", "Yes")
    assert face_service.enhancer_settings() == (1.5, 1000, 70, True)
    monkeypatch.setenv("ENHANCER_SHARPEN", "0")
    assert face_service.enhancer_settings()[3] is False


def test_new_symbols_are_part_of_the_abi():
    from frp_amd import native
    lib = native.load_library()
    for name in ("frp_enhance_pixels", "frp_encode_jpeg_enhanced"):
        assert name in native.ABI_SYMBOLS and hasattr(lib, name)
