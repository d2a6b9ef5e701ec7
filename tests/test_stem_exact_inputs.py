"""The conditions tests/test_gpu_stem_exact.py rests on, asserted on its planted weights and its reference alone (no device): the
stems' arithmetic is exact in fp32, the one rounding per layer meets ties, folding keeps the planted values, and every shape of the
table reaches the staging path, guard and loop it is there for.  The predicates of stem12_u8_kernel are restated here from its
constants (tile 4 x 32, patch 19 rows x 131 pixels, one pixel of slack for the unaligned dword path), not parsed from the source."""
import numpy as np
import pytest

import test_gpu_conv_exact as gx
import test_gpu_stem_exact as sx

CU = sx.REF_CU
SHAPES = [sx.resolve(s, CU) for s in sx.SHAPES]
ids = ["x".join(map(str, s)) for s in SHAPES]


def test_the_table_at_256_cus():
    assert SHAPES == [(1, 32, 32), (3, 97, 131), (2, 64, 256), (2, 64, 257), (9, 256, 512), (7, 256, 544)]
    assert sx.ODD_STRIDES == (3, 97, 131) and sx.FAST_TILES == (2, 64, 257)


def test_planted_weights_are_what_the_issue_says():
    w1, b1, w2, b2 = (a.astype(np.float64) for a in sx.planted("exact"))
    assert w1.shape == (32, 3, 3, 8) and w2.shape == (64, 3, 3, 32) and b1.shape == (32,) and b2.shape == (64,)
    assert not w1[..., 3:].any() and set(np.unique(w1[..., :3])) == set(range(-4, 5)) and set(np.unique(w2)) == {-1, 0, 1}
    assert np.array_equal(b1, np.round(b1)) and -8 <= b1.min() and b1.max() <= 24
    assert np.array_equal(b2, np.round(b2)) and -64 <= b2.min() and b2.max() <= 64
    w1, b1, w2, b2 = (a.astype(np.float64) for a in sx.planted("stamp"))
    for j in range(32):
        hot = np.argwhere(w1[j])
        assert hot.tolist() == ([[j // 9, (j // 3) % 3, j % 3]] if j < 27 else []) and w1[j].sum() == (j < 27) and b1[j] == (j < 27)
    for j in range(64):
        assert np.argwhere(w2[j]).tolist() == [[1, 1, j % 32]] and w2[j, 1, 1, j % 32] == 1
    assert not b2.any()


@pytest.mark.parametrize("kind", ["exact", "stamp"])
def test_folding_keeps_the_planted_values(kind):
    """(d) fold_layer on the edited raw weights, then the hook: exactly the planted weights and biases; every other layer untouched"""
    from frp_amd import netspec, weights
    raw, hook = sx.planted_raw_and_hook(kind)
    plain = weights.make_synthetic_raw(7, sx.DET_BLOCKS, sx.EMB_BLOCKS)
    layers = netspec.detector_layers(sx.DET_BLOCKS)
    w1, b1, w2, b2 = sx.planted(kind)
    for layer, w, b in ((layers[0], w1, b1), (layers[1], w2, b2)):
        w16, bias, slope = weights.fold_layer(raw, layer)
        got = hook(layer, w16)
        assert got.dtype == np.float16 and np.array_equal(got.view(np.uint16), w.view(np.uint16))
        assert bias.dtype == np.float32 and np.array_equal(bias.view(np.uint32), b.view(np.uint32)) and slope is None
    assert (layers[0].name, layers[0].cin, layers[0].cout, layers[0].stride) == ("det.stem1.conv", 8, 32, 2)
    assert (layers[1].name, layers[1].cin, layers[1].cout, layers[1].stride, layers[1].src) == ("det.stem2.conv", 32, 64, 2, layers[0].dst)
    for layer in layers[2:] + netspec.iresnet_layers(sx.EMB_BLOCKS):
        a, b = weights.fold_layer(raw, layer), weights.fold_layer(plain, layer)
        assert hook(layer, a[0]) is a[0] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _multiples_of_2_8(a):
    return bool(np.array_equal(a * 256.0, np.round(a * 256.0)))


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_stem_arithmetic_is_exact_and_the_rounding_is_exercised(shape):
    B, H, W = shape
    w1, b1, w2, b2 = sx.planted("exact")
    ref = sx.reference(B, H, W, "exact")
    x = sx.canvas_input(sx.frames_for(B, H, W))
    # the input: odd multiples of 2^-8 inside (-1, 1), exact in fp16; the letterbox is u8 zero, not the conv's zero padding
    assert np.array_equal(x.astype(np.float16).astype(np.float64), x) and np.all(np.round(x * 256.0) % 2 == 1) and np.abs(x).max() <= 255 / 256
    if (H % 32) or (W % 32):
        assert np.all(x[:, H:] == sx.LETTERBOX) and np.all(x[:, :, W:] == sx.LETTERBOX)
    # (a) stem1: every partial sum in any order is a multiple of 2^-8 of magnitude below 2^16, hence exact in fp32's 24 bits
    bound1 = sx.conv3x3_s2(np.abs(x), np.abs(w1), np.abs(b1)).max()
    assert bound1 <= 27 * 4 * 255 / 256 + 24 < 132 and _multiples_of_2_8(ref["y1"])
    # (b) stem2 from the fp16 stem1 map: multiples of 2^-8 again, bounded by 288 taps x max |w2| x max(stem1) (+ the bias)
    s1 = ref["s1"].astype(np.float64)
    assert _multiples_of_2_8(s1) and s1.max() <= bound1
    bound2 = 288 * np.abs(w2.astype(np.float64)).max() * s1.max() + np.abs(b2).max()
    assert bound2 <= 38016 + 64 < 65536 and _multiples_of_2_8(ref["y2"]) and np.abs(ref["y2"]).max() <= bound2
    # (c) of the outputs ReLU leaves to the rounding, a share lies exactly on an fp16 tie; ReLU does not empty the test
    for y, out, cap in ((ref["y1"], ref["s1"], 0.10), (ref["y2"], ref["s2"], 0.03)):
        pos = y > 0
        ties = gx.tie_mask(y, y.astype(np.float16))
        print(f"{B}x{H}x{W}: positive {pos.mean():.3f}, ties among them {ties[pos].mean():.3f}")
        assert pos.mean() >= 0.40 and ties[pos].mean() >= cap
        assert np.all((out[ties & pos].view(np.uint16) & 1) == 0)          # numpy's cast rounds them to even
        assert np.array_equal(out[~pos], np.zeros(int((~pos).sum()), np.float16)) and not np.signbit(out).any()


def test_reference_is_the_oracles_convolution():
    """the one-matmul-per-tap reference against the oracle's input blob and torch's float64 conv2d: same canvas, colour order, padding
    and stride phase, to the last bit (every sum is exact in float64 in any order)"""
    import torch
    import torch.nn.functional as F
    from oracle import network as onet
    B, H, W = sx.ODD_STRIDES
    w1, b1, w2, b2 = sx.planted("exact")
    ref = sx.reference(B, H, W, "exact")
    x = onet.det_blob(sx.frames_for(B, H, W), (sx.round_up(H, 32), sx.round_up(W, 32))).double()
    assert np.array_equal(x.permute(0, 2, 3, 1).numpy(), sx.canvas_input(sx.frames_for(B, H, W)))
    for inp, w, b, want in ((x, w1[..., :3], b1, ref["y1"]), (torch.from_numpy(ref["s1"].astype(np.float64)).permute(0, 3, 1, 2), w2, b2, ref["y2"])):
        wt = torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2)
        y = F.conv2d(inp, wt, torch.from_numpy(b.astype(np.float64)), stride=2, padding=1).permute(0, 2, 3, 1).numpy()
        assert np.array_equal(y, want)


@pytest.mark.parametrize("shape", [sx.ODD_STRIDES, sx.FAST_TILES], ids=sx.shape_id)
def test_tap_stamp_is_the_shifted_input_plane(shape):
    B, H, W = shape
    ref = sx.reference(B, H, W, "stamp")
    x = np.pad(sx.canvas_input(sx.frames_for(B, H, W)), ((0, 0), (1, 1), (1, 1), (0, 0)))
    Ho, Wo = ref["s1"].shape[1:3]
    for j in range(27):
        kh, kw, c = j // 9, (j // 3) % 3, j % 3
        assert np.array_equal(ref["s1"][..., j].astype(np.float64), 1 + x[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, c])
    assert ref["s1"][..., :27].min() > 0 and not ref["s1"][..., 27:].any()      # (1 + v >= 1/256 inside the canvas, 1 on its padding)
    assert np.array_equal(ref["s1"].astype(np.float64), np.maximum(ref["y1"], 0))                # nothing rounds
    assert np.array_equal(ref["s2"], np.concatenate([ref["s1"][:, ::2, ::2], ref["s1"][:, ::2, ::2]], axis=-1))


# ---------------------------------------------------------------------------------------------------------------- (e) shape claims

def tile_interior(H, W, y2_0, x2_0):
    """prefetch time: the unaligned-dword ("fast") staging path, for BGR frames"""
    iy0, ix0 = 4 * y2_0 - 3, 4 * x2_0 - 3
    return iy0 >= 0 and iy0 + sx.S12_PATCH_ROWS <= H and ix0 >= 0 and ix0 + sx.S12_PATCH_PIX + sx.S12_SLACK <= W


def interior(H, W, y2_0, x2_0):
    """unpack time: the per-element path skips its padding / letterbox logic"""
    iy0, ix0 = 4 * y2_0 - 3, 4 * x2_0 - 3
    return iy0 >= 0 and iy0 + sx.S12_PATCH_ROWS <= H and ix0 >= 0 and ix0 + sx.S12_PATCH_PIX <= W


def slow_path_dwords(B, H, W):
    """[(lo, hi)] byte ranges, relative to the first byte of the batch (4-byte aligned, as device allocations are), of the aligned
    dwords the per-element path fetches: 99 per patch row from the row's clamped address rounded down"""
    out = []
    for b in range(B):
        for (y2_0, x2_0) in sx.stem12_tiles(H, W):
            if tile_interior(H, W, y2_0, x2_0):
                continue
            for pr in range(sx.S12_PATCH_ROWS):
                iy = min(max(4 * y2_0 - 3 + pr, 0), H - 1)
                a = b * H * W * 3 + iy * W * 3 + (4 * x2_0 - 3) * 3
                al = a - a % 4
                out += [(al + 4 * d, al + 4 * d + 4) for d in range(sx.S12_ROW_DWORDS)]
    return out


def fast_path_last_byte(B, H, W):
    """one past the last byte any unaligned dword of the fast path reads"""
    ends = [b * H * W * 3 + (4 * y - 3 + sx.S12_PATCH_ROWS - 1) * W * 3 + (4 * x - 3) * 3 + 4 * sx.S12_ROW_DWORDS
            for b in range(B) for (y, x) in sx.stem12_tiles(H, W) if tile_interior(H, W, y, x)]
    return max(ends) if ends else None


def test_shape_1x32x32_is_the_smallest_canvas_all_border_without_letterbox():
    """(a canvas is a multiple of 32, so a stem2 map has at least 8 rows: two tiles of 4 rows is the fewest a launch can have)"""
    B, H, W = SHAPES[0]
    assert sx.stem12_tiles(H, W) == [(0, 0), (4, 0)] and not any(interior(H, W, y, x) for (y, x) in sx.stem12_tiles(H, W))
    assert (sx.round_up(H, 32), sx.round_up(W, 32)) == (H, W) and B * 2 < 2 * CU


def test_shape_3x97x131_has_every_alignment_letterbox_ragged_tiles_and_both_buffer_ends():
    B, H, W = SHAPES[1]
    assert W * 3 == 393 and {(y * W * 3) % 4 for y in range(H)} == {0, 1, 2, 3} and (H * W * 3) % 4 != 0
    assert (sx.round_up(H, 32), sx.round_up(W, 32)) == (128, 160) and H < 128 and W < 160
    assert [x for (y, x) in sx.stem12_tiles(H, W) if y == 0] == [0, 32] and 160 // 4 - 32 == 8         # the second tile column: 8 of 32
    assert 160 // 2 == 80 and 80 % sx.ST_COLS == 16                                                    # stem_u8: 64 + 16 of 64
    assert not any(tile_interior(H, W, y, x) or interior(H, W, y, x) for (y, x) in sx.stem12_tiles(H, W))
    end = B * H * W * 3
    dw = slow_path_dwords(B, H, W)
    assert any(hi <= 0 for lo, hi in dw) and any(lo < end < hi for lo, hi in dw)     # dwords before the batch; one across its last byte


def test_shape_2x64x256_skips_the_padding_logic_on_the_per_element_path():
    B, H, W = SHAPES[2]
    tiles = sx.stem12_tiles(H, W)
    assert not any(tile_interior(H, W, y, x) for (y, x) in tiles)
    assert [(y, x) for (y, x) in tiles if interior(H, W, y, x)] == [(4, 32), (8, 32), (12, 32)]
    assert 4 * 32 - 3 + sx.S12_PATCH_PIX == W                                        # the patch ends on the frame's last pixel


def test_shape_2x64x257_takes_the_dword_path_with_no_slack_left():
    B, H, W = SHAPES[3]
    tiles = sx.stem12_tiles(H, W)
    assert [(y, x) for (y, x) in tiles if tile_interior(H, W, y, x)] == [(4, 32), (8, 32), (12, 32)]
    assert 4 * 32 - 3 + sx.S12_PATCH_PIX + sx.S12_SLACK == W and 4 * 12 - 3 + sx.S12_PATCH_ROWS == H
    assert fast_path_last_byte(B, H, W) == B * H * W * 3                             # the last row's 99th dword ends on the batch's last byte
    assert sx.round_up(W, 32) == 288 and [x for (y, x) in tiles if y == 0] == [0, 32, 64] and 288 // 4 - 64 == 8
    # ... and a one-pixel narrower guard (`+ 0` for the slack) would send the tiles of shape 2 down this path, 3 bytes past each row
    assert fast_path_last_byte(*SHAPES[2]) is None


def _walk(B, H, W, cu):
    """per persistent workgroup that gets more than one tile: whether each of its tiles takes the dword path, in order"""
    per_frame = sx.stem12_tiles(H, W)
    n, grid = B * len(per_frame), 2 * cu
    assert n > grid
    return [[tile_interior(H, W, *per_frame[t % len(per_frame)]) for t in range(wg, n, grid)] for wg in range(n - grid)]


def test_shape_9x256x512_outnumbers_the_persistent_workgroups():
    B, H, W = SHAPES[4]
    assert len(sx.stem12_tiles(H, W)) == 64 and B == 2 * CU // 64 + 1 == 9 and B * 64 > 2 * CU and B <= 32      # (Engine's default max_batch)
    walks = _walk(B, H, W, CU)
    assert len(walks) == 64 and all(len(w) == 2 for w in walks)
    second = [w[1] for w in walks]
    assert sum(second) == 30 and len(second) - sum(second) == 34         # the tiles that go through the prefetch-ahead loop: both paths
    assert all(w[0] == w[1] for w in walks)                              # 2 * CU is a multiple of 64: a workgroup stays on one path ...


def test_shape_7x256x544_switches_paths_inside_a_workgroup():
    B, H, W = SHAPES[5]
    assert len(sx.stem12_tiles(H, W)) == 80 and B == 7 and B <= 32
    walks = _walk(B, H, W, CU)                                           # ... which is why this shape is here
    assert len(walks) == 48 and [True, False] in walks and [False, True] in walks and [True, True] in walks and [False, False] in walks
