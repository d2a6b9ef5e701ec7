"""Zero-tolerance tests of the detector's u8 stem kernels (csrc/stem_kernel.hip: stem_u8_kernel, stem12_u8_kernel).

Every frame goes through them first, yet they cannot be reached through frp_conv2d_nhwc, and the tests that do run them look at head
maps, three stride-2 stages and a dozen ReLUs later.  Here the two stem layers carry planted integer weights: the input
(u - 127.5) / 128 is an odd multiple of 2^-8, so every product and partial sum is a multiple of 2^-8 below 2^16 - exact in fp32 in any
order - and each layer has exactly ONE rounding (fp32 -> fp16, nearest even).  The kernels owe a float64 reference its bits.  The
tensors are read back with Engine.det_prefix: op 1's output is stem12_u8_kernel's by default; with FRP_NO_FUSED_STEM12 op 0's is
stem_u8_kernel's and op 1's the generic stride-2 kernel's.

tests/test_stem_exact_inputs.py imports the planted weights, the reference and the shape list from here and proves, without a
device, the conditions the comparison rests on and what each shape reaches.  Nothing device-specific is imported at module level.
"""
import functools

import numpy as np
import pytest

from test_gpu_conv_exact import _assert_bits

pytestmark = pytest.mark.gpu

DET_BLOCKS, EMB_BLOCKS = (1, 2, 2, 2), (1, 1, 1, 1)
LETTERBOX = -255.0 / 256.0            # u8 zero in the normalised domain

# stem12_u8_kernel's geometry (restated, not parsed): stem2 tiles of 4 x 32 outputs; a tile reads a patch of 19 rows x 131 pixels whose
# origin is 3 pixels up and left of 4 x the tile's; the unaligned dword path wants one more pixel to the right of the patch in the frame
S12_ROWS, S12_COLS, S12_PATCH_ROWS, S12_PATCH_PIX, S12_SLACK, S12_ROW_DWORDS = 4, 32, 19, 131, 1, 99
ST_COLS = 64                          # stem_u8_kernel: 4 x 64 stem1 outputs per workgroup
REF_CU = 256                          # the CU count the shape table is worked out for (tests/test_stem_exact_inputs.py)


def batch_for(tiles_per_frame, cu):
    """the smallest batch whose stem12 tiles outnumber the 2 * CU persistent workgroups"""
    return 2 * cu // tiles_per_frame + 1


# (B, H, W); B None: batch_for(the frame's tile count, the device's CU count).  What each shape reaches: DESIGN.md 4.7, asserted by
# tests/test_stem_exact_inputs.py.  The last row is this file's addition: with 80 tiles per frame a workgroup's second tile is another
# position than its first, so single workgroups go from the dword path to the per-element path and back.
SHAPES = [(1, 32, 32), (3, 97, 131), (2, 64, 256), (2, 64, 257), (None, 256, 512), (None, 256, 544)]
ODD_STRIDES, FAST_TILES = SHAPES[1], SHAPES[3]

ROUTES = {"stem12": (False, 2), "stem_u8": (True, 1), "stem_u8+generic-s2": (True, 2)}    # FRP_NO_FUSED_STEM12, det_prefix's n_ops


def round_up(v, m):
    return (v + m - 1) // m * m


def stem12_tiles(H, W):
    """[(y2_0, x2_0)] of one frame's stem12 tiles in the kernel's order (x fastest)"""
    Ho2, Wo2 = round_up(H, 32) // 4, round_up(W, 32) // 4
    return [(y, x) for y in range(0, Ho2, S12_ROWS) for x in range(0, Wo2, S12_COLS)]


def resolve(shape, cu):
    B, H, W = shape
    return (batch_for(len(stem12_tiles(H, W)), cu) if B is None else B), H, W


def shape_id(shape):
    return "x".join("Bstar" if v is None else str(v) for v in shape)


def _ro(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def planted(kind="exact"):
    """-> w1 [32][3][3][8] fp16, b1 [32] fp32, w2 [64][3][3][32] fp16, b2 [64] fp32 of the two stem layers.
    "exact": stem1 integers in [-4, 4] on the 3 real channels with biases in [-8, 24], stem2 in {-1, 0, 1} with biases in [-64, 64].
    "stamp": stem1 cout j < 27 one-hot on tap (kh, kw, c) = (j // 9, (j // 3) % 3, j % 3) with bias 1 - channel j of the map is
    1 + the shifted, strided input plane, positive everywhere -, the other couts zero; stem2 cout j one-hot on the centre tap of
    stem1 channel j % 32, bias 0."""
    w1, w2 = np.zeros((32, 3, 3, 8), np.float16), np.zeros((64, 3, 3, 32), np.float16)
    if kind == "exact":
        rng = np.random.default_rng(11)
        w1[..., :3] = rng.integers(-4, 5, size=(32, 3, 3, 3))
        b1 = rng.integers(-8, 25, size=32).astype(np.float32)
        w2[:] = rng.integers(-1, 2, size=w2.shape)
        b2 = rng.integers(-64, 65, size=64).astype(np.float32)
    else:
        b1, b2 = np.zeros(32, np.float32), np.zeros(64, np.float32)
        for j in range(27):
            w1[j, j // 9, (j // 3) % 3, j % 3] = 1
            b1[j] = 1
        for j in range(64):
            w2[j, 1, 1, j % 32] = 1
    return tuple(_ro(a) for a in (w1, b1, w2, b2))


def planted_raw_and_hook(kind="exact"):
    """the synthetic raw weights with the stems' biases planted through their BatchNorm entries (running_mean 0 and neither a conv bias
    nor a pre-BN: the folded bias is beta), and the w16_hook that substitutes the stems' folded weights"""
    from frp_amd import netspec, weights
    w1, b1, w2, b2 = planted(kind)
    s1, s2 = netspec.detector_layers(DET_BLOCKS)[:2]
    raw = dict(weights.make_synthetic_raw(7, DET_BLOCKS, EMB_BLOCKS))
    for layer, b in ((s1, b1), (s2, b2)):
        assert layer.post_bn and not layer.pre_bn and not layer.conv_bias
        raw[layer.post_bn + ".bias"] = b.copy()
        raw[layer.post_bn + ".running_mean"] = np.zeros_like(b)
    subst = {s1.name: w1, s2.name: w2}

    def hook(layer, w16):
        w = subst.get(layer.name)
        if w is None:
            return w16
        assert w.shape == w16.shape and w16.dtype == np.float16
        return w.copy()
    return raw, hook


_BLOBS = {}


def planted_blob(kind="exact"):
    if kind not in _BLOBS:
        from frp_amd import weights
        raw, hook = planted_raw_and_hook(kind)
        _BLOBS[kind] = weights.pack_blob(raw, DET_BLOCKS, EMB_BLOCKS, w16_hook=hook)
    return _BLOBS[kind]


@functools.lru_cache(maxsize=None)
def frames_for(B, H, W):
    return _ro(np.random.default_rng([3, B, H, W]).integers(0, 256, size=(B, H, W, 3), dtype=np.uint8))


def canvas_input(frames):
    """BGR u8 [B, H, W, 3] -> the detector's float64 input [B, Hc, Wc, 3] in RGB order on the letterbox canvas"""
    B, H, W, _ = frames.shape
    x = np.full((B, round_up(H, 32), round_up(W, 32), 3), LETTERBOX)
    x[:, :H, :W] = (frames[..., ::-1].astype(np.float64) - 127.5) / 128.0
    return x


def conv3x3_s2(x, w, bias):
    """float64 3x3 stride-2 pad-1 conv (zero padding) + bias, NHWC, w [cout][kh][kw][cin]: one matmul per tap"""
    B, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    acc = np.zeros((B * Ho * Wo, w.shape[0]))
    for kh in range(3):
        for kw in range(3):
            acc += np.ascontiguousarray(xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, :]).reshape(-1, C) @ w[:, kh, kw, :C].astype(np.float64).T
    return acc.reshape(B, Ho, Wo, -1) + bias.astype(np.float64)


def round_relu(y):
    """ONE rounding to fp16 (numpy: nearest even), then ReLU (0 is +0)"""
    y16 = y.astype(np.float16)
    return np.where(y16 > 0, y16, np.float16(0))


@functools.lru_cache(maxsize=None)
def reference(B, H, W, kind="exact"):
    """-> dict: y1 / y2 the float64 sums + bias of stem1 / stem2 (stem2 from the fp16 stem1 map), s1 / s2 their fp16 maps"""
    w1, b1, w2, b2 = planted(kind)
    y1 = conv3x3_s2(canvas_input(frames_for(B, H, W)), w1, b1)
    s1 = round_relu(y1)
    y2 = conv3x3_s2(s1.astype(np.float64), w2, b2)
    return {k: _ro(v) for k, v in dict(y1=y1, s1=s1, y2=y2, s2=round_relu(y2)).items()}


# ---------------------------------------------------------------------------------------------------------------- device side

def _device_shape(engine, shape):
    import torch
    B, H, W = resolve(shape, torch.cuda.get_device_properties(0).multi_processor_count)
    assert B <= engine.max_batch, f"the batch {B} of {shape_id(shape)} does not fit the engine's max_batch {engine.max_batch}"
    return B, H, W


def _route(monkeypatch, route):
    two_kernels, n_ops = ROUTES[route]
    monkeypatch.delenv("FRP_NO_FUSED_STEM", raising=False)
    if two_kernels:
        monkeypatch.setenv("FRP_NO_FUSED_STEM12", "1")
    else:
        monkeypatch.delenv("FRP_NO_FUSED_STEM12", raising=False)
    return n_ops


def _check(engine, monkeypatch, shape, route, kind):
    B, H, W = _device_shape(engine, shape)
    n_ops = _route(monkeypatch, route)
    ref = reference(B, H, W, kind)
    engine.load_weights(planted_blob(kind))
    engine.upload_frames(frames_for(B, H, W))
    out = engine.det_prefix(n_ops)
    _assert_bits(out, ref["s1" if n_ops == 1 else "s2"], f"{B}x{H}x{W} route {route} ({kind} weights)")


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_stems_return_the_reference_bits(engine, monkeypatch, shape, route):
    _check(engine, monkeypatch, shape, route, "exact")


@pytest.mark.parametrize("route", ["stem_u8", "stem12"])
@pytest.mark.parametrize("shape", [ODD_STRIDES, FAST_TILES], ids=shape_id)
def test_tap_stamp(engine, monkeypatch, shape, route):
    """Diagnosis for a red exact set: channel j < 27 of the stem1 map is 1 + input plane j % 3 shifted by tap (j // 9, (j // 3) % 3) -
    nothing rounds, ReLU hides nothing -, and through the fused kernel stem2's channel j is stem1's channel j % 32 at every second
    pixel.  The first mismatch names the tap, the colour and the pixel."""
    _check(engine, monkeypatch, shape, route, "stamp")


def test_prefix_of_one_op_needs_the_two_kernel_path(engine, monkeypatch):
    """While both stems run as one kernel the stem1 map never reaches memory: no tensor to return, and no stale buffer instead"""
    from frp_amd import native
    B, H, W = ODD_STRIDES
    engine.load_weights(planted_blob("exact"))
    engine.upload_frames(frames_for(B, H, W))
    _route(monkeypatch, "stem12")
    with pytest.raises(native.FrpError, match="FRP_NO_FUSED_STEM12") as err:
        engine.det_prefix(1)
    assert err.value.code == -1                                      # FRP_ERR_INVALID
    assert engine.det_prefix(2).shape == (B, 32, 40, 64)             # (the handle is none the worse for it)
    _route(monkeypatch, "stem_u8")
    assert engine.det_prefix(1).shape == (B, 64, 80, 32)


@pytest.mark.selfcheck
@pytest.mark.parametrize("shape", [ODD_STRIDES, FAST_TILES], ids=shape_id)
def test_rgb_frames_give_the_head_maps_of_bgr_frames(engine, monkeypatch, shape):
    """det_prefix stages BGR only.  RGB frames (flag bit 1) are swapped at staging time and must stay off the dword path, which copies
    the frame's byte order: the same head maps as the BGR frames, bit for bit, and the stem12 map they both start from is the
    reference's."""
    B, H, W = shape
    _route(monkeypatch, "stem12")
    engine.load_weights(planted_blob("exact"))
    frames = frames_for(B, H, W)
    engine.detect(frames, max_faces=4, det_thresh=0.5)
    bgr = engine.head_maps()
    engine.detect(frames[..., ::-1].copy(), max_faces=4, det_thresh=0.5, flags=2)
    rgb = engine.head_maps()
    engine.upload_frames(frames)
    stem = engine.det_prefix(2)
    assert len(bgr) == len(rgb) == 3
    for lv, (a, b) in enumerate(zip(bgr, rgb)):
        print(f"{shape_id(shape)} level {lv}: finite {np.isfinite(a).mean():.3f}, max |finite| {np.abs(a[np.isfinite(a)]).max():.1f}")
        assert np.isfinite(a).all()                     # (a float64 pass of these weights peaks near 4600: nothing saturates into agreement)
        assert np.array_equal(a, b), f"head map {lv}: {int((a != b).sum())} of {a.size} elements differ"
    _assert_bits(stem, reference(B, H, W)["s2"], f"{shape_id(shape)} stem12 map")
