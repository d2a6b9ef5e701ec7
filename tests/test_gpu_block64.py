"""The fused residual-block kernel (csrc/conv3x3_block64.hip): out = act2(conv2(act1(conv1(x))) + x), both convs 3x3 stride 1 64 -> 64,
in one launch with the intermediate tensor in LDS only.  Its whole parity story is "the same bits as the two launches it replaces":
no tolerance anywhere in this file.

Kernel level: Engine.conv_block64 against two Engine.conv2d calls (uint16 views compared with np.array_equal) on the smallest maps at
which strips, halos and segment seams can go wrong, and - independent of the unfused kernels - against a float64 reference on the
integer operands of tests/test_gpu_conv_exact.py, whose every partial sum is exact in fp32.  frp_conv_block64 itself puts x and out
between NaN-filled guard regions on the device and pre-fills out with NaNs: a read outside x, a write outside out or a pixel never
written fails the call or the comparison.

Engine level: both networks with the fused launch against FRP_NO_BLOCK_FUSE=1 - bits, launch and FLOP counters, per-op hashes,
threshold mode, replayed graphs."""
import functools

import numpy as np
import pytest

import test_gpu_conv_exact as gx
from conftest import get_raw_and_blob

pytestmark = pytest.mark.gpu

RELU, PRELU, BORDER = 1, 2, 1
# (activation 1, flags 1, activation 2): the detector's block and the embedder's
VARIANTS = {"det": (RELU, 0, RELU), "emb": (PRELU, BORDER, 0)}
# (N, H, W): what it exercises
SHAPES = [
    (1, 2, 2),       # smallest map border classes allow
    (2, 3, 29),      # one ragged strip
    (1, 5, 30),      # exactly one full strip
    (1, 4, 31),      # second strip one column wide
    (3, 9, 61),      # three strips, ragged last, H not a multiple of the rows per step, image seams
    (2, 8, 60),      # two full strips
    (1, 33, 90),     # many steps
    (5, 56, 56),     # segment seams
    (1, 16, 480),    # 16 strips
]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@functools.lru_cache(maxsize=None)
def _normal_operands(variant, shape):
    """standard-normal operands scaled like a trained layer's; every image its own content"""
    N, H, W = shape
    act1, flags1, act2 = VARIANTS[variant]
    rng = np.random.default_rng([3, act1, N, H, W])
    x = rng.standard_normal((N, H, W, 64)).astype(np.float16)
    w1 = (rng.standard_normal((64, 3, 3, 64)) / 24).astype(np.float16)
    w2 = (rng.standard_normal((64, 3, 3, 64)) / 24).astype(np.float16)
    bias1 = rng.standard_normal((9, 64) if flags1 & BORDER else (64,)).astype(np.float32)
    bias2 = rng.standard_normal(64).astype(np.float32)
    slope1 = rng.uniform(0.05, 0.5, 64).astype(np.float32) if act1 == PRELU else None
    return x, w1, bias1, slope1, w2, bias2


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_block_returns_the_bits_of_its_two_launches(engine, variant, shape):
    act1, flags1, act2 = VARIANTS[variant]
    x, w1, bias1, slope1, w2, bias2 = _normal_operands(variant, shape)
    mid = engine.conv2d(x, w1, bias1, act=act1, slope=slope1, flags=flags1)
    want = engine.conv2d(mid, w2, bias2, act=act2, res=x)
    got = engine.conv_block64(x, w1, bias1, w2, bias2, act1=act1, act2=act2, slope1=slope1, flags1=flags1)
    assert not np.isnan(want).any()
    bad = np.argwhere((_bits(got) != _bits(want)).any(axis=3))
    assert bad.size == 0, f"{len(bad)} pixels differ, first (n, y, x) = {bad[0].tolist()}"
    assert np.array_equal(_bits(engine.conv_block64(x, w1, bias1, w2, bias2, act1=act1, act2=act2, slope1=slope1, flags1=flags1)), _bits(got))


@functools.lru_cache(maxsize=None)
def _exact_block(variant, shape):
    """conv1's operands and its rounded result from test_gpu_conv_exact's generator (integers: every partial sum exact in fp32), conv2's
    weights drawn the same way; the float64 reference of the block with the intermediate rounded to fp16 where the kernels round it"""
    import torch
    import torch.nn.functional as F
    N, H, W = shape
    act1, flags1, act2 = VARIANTS[variant]
    ops = gx.exact_operands(gx._case(N, H, W, 64, 64, 3, 1, act1, False, flags1), 0, "exact")
    rng = np.random.default_rng([11, act1, N, H, W])
    w2 = rng.choice(np.arange(-1, 2), size=(64, 3, 3, 64), p=[0.3, 0.4, 0.3]).astype(np.float16)
    bias2 = rng.integers(-8, 9, size=64).astype(np.float32)
    mid = ops["ref_out"]
    assert np.array_equal(mid.astype(np.float64), ops["ref"])                   # the intermediate's rounding is the identity
    mt = torch.from_numpy(mid.astype(np.float64)).permute(0, 3, 1, 2)
    wt = torch.from_numpy(w2.astype(np.float64)).permute(0, 3, 1, 2)
    y = F.conv2d(mt, wt, None, padding=1).permute(0, 2, 3, 1).numpy() + bias2.astype(np.float64) + ops["x"].astype(np.float64)
    # multiples of 1/4 (PReLU slopes 1/2, 1/4) far below 2^22: every partial sum of conv2 is exact in fp32 as well
    assert float(F.conv2d(mt.abs(), wt.abs(), None, padding=1).max()) + 8 + 2 < 2 ** 22
    if act2 == RELU:
        y = np.maximum(y, 0)
    with np.errstate(over="ignore"):
        return ops, w2, bias2, y.astype(np.float16)


@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 9, 61), (1, 4, 31), (2, 30, 56)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fused_block_equals_the_float64_reference_on_exact_operands(engine, variant, shape):
    act1, flags1, act2 = VARIANTS[variant]
    ops, w2, bias2, want = _exact_block(variant, shape)
    got = engine.conv_block64(ops["x"], ops["w"], ops["bias"], w2, bias2, act1=act1, act2=act2, slope1=ops["slope"], flags1=flags1)
    bad = np.argwhere((_bits(got) != _bits(want)).any(axis=3))
    assert bad.size == 0, f"{len(bad)} pixels differ, first (n, y, x) = {bad[0].tolist()}"


def test_block_entry_point_refuses_what_the_kernel_does_not_cover(engine):
    from frp_amd import native
    x, w1, bias1, slope1, w2, bias2 = _normal_operands("det", (1, 2, 2))
    with pytest.raises(native.FrpError):
        engine.conv_block64(x, w1, bias1, w2, bias2, act1=RELU, act2=0)                    # no such epilogue pair
    with pytest.raises(native.FrpError):
        engine.conv_block64(x, w1, bias1, w2, bias2, act1=PRELU, act2=0, flags1=0, slope1=bias2)


# ---------------------------------------------------------------------------------------------------------------- engine level
def _frames(rng, B, H, W):
    base = rng.integers(0, 256, size=(B, H // 8 + 1, W // 8 + 1, 3), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(base, 8, axis=1), 8, axis=2)[:, :H, :W])


def test_embedder_with_fused_blocks_is_bit_identical(fresh_engine, monkeypatch):
    """blocks (2, 1, 1, 1): emb.layer1.1 is the one eligible block.  37 and 8 faces at 56 x 56 are far below the maps on which the launch
    pays: the default rule leaves the pair alone (equal launches), FRP_BLOCK_FUSE_ALL=1 fuses it (one launch fewer); always the bits
    and the FLOPs of FRP_NO_BLOCK_FUSE=1; five repeated calls (the later ones replayed graphs) return the same bits."""
    engine = fresh_engine
    rng = np.random.default_rng(31)
    chips = rng.integers(0, 256, size=(37, 112, 112, 3), dtype=np.uint8)
    raw, blob = get_raw_and_blob((1, 1, 1, 1), (2, 1, 1, 1))
    engine.load_weights(blob)
    out = {}
    for mode, env in (("default", {}), ("all", {"FRP_BLOCK_FUSE_ALL": "1"}), ("separate", {"FRP_NO_BLOCK_FUSE": "1"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for n in (37, 8):
            engine.reset_counters()
            e = engine.embed_aligned(chips[:n])
            c = engine.counters()
            out[mode, n] = (e, c["emb_conv_launches"], c["emb_conv_flops"])
            if mode == "all":
                for _ in range(5):
                    assert np.array_equal(engine.embed_aligned(chips[:n]), e)
        for k in env:
            monkeypatch.delenv(k)
    for n in (37, 8):
        b, lb, fb = out["separate", n]
        assert out["all", n][1] == lb - 1 and out["default", n][1] == lb
        for mode in ("default", "all"):
            assert np.array_equal(out[mode, n][0], b), (mode, n)
            assert out[mode, n][2] == fb


@pytest.mark.parametrize("B,H,W,force", [(4, 1080, 1920, False), (2, 256, 384, True)], ids=["4x1080p-default", "2x256x384-all"])
def test_detector_with_the_fused_block_is_bit_identical(fresh_engine, monkeypatch, B, H, W, force):
    """det.layer1.0 as one launch (4 x 1080p: by the default rule; the small frames: FRP_BLOCK_FUSE_ALL=1): the head maps of
    FRP_NO_BLOCK_FUSE=1, one launch fewer, the same FLOPs; with the per-op hashes on the pair runs as two launches, so every op slot is
    written and equals the unfused pass's."""
    engine = fresh_engine
    rng = np.random.default_rng(59)
    raw, blob = get_raw_and_blob((1, 1, 1, 1), (1, 1, 1, 1))
    engine.load_weights(blob)
    engine.upload_frames(_frames(rng, B, H, W))
    if force:
        monkeypatch.setenv("FRP_BLOCK_FUSE_ALL", "1")

    def run():
        engine.reset_counters()
        engine.detect_resident((H, W), max_faces=8, det_thresh=0.5)
        c = engine.counters()
        return [h.copy() for h in engine.head_maps()], c["det_conv_launches"], c["det_conv_flops"]

    fused = [run() for _ in range(3)]                      # launch by launch, capturing, replayed
    engine.det_hashes(True, fetch=False)
    try:
        run()
        h_fused = engine.det_hashes()
        monkeypatch.setenv("FRP_NO_BLOCK_FUSE", "1")
        run()
        h_sep = engine.det_hashes()
    finally:
        engine.det_hashes(False, fetch=False)
    sep = run()
    assert fused[0][1] == sep[1] - 1 and fused[0][2] == sep[2]
    for heads, launches, flops in fused:
        assert launches == fused[0][1]
        for a, b in zip(heads, sep[0]):
            assert np.array_equal(_bits(a), _bits(b))
    n_ops = int(np.count_nonzero(h_sep))
    assert n_ops >= 20 and np.array_equal(h_fused, h_sep) and len(set(h_sep[h_sep != 0].tolist())) == n_ops


def test_threshold_mode_and_replayed_graphs_with_fused_blocks(fresh_engine, monkeypatch):
    """the whole pipeline with the face count on the device (below the embedder's capacity) and every eligible block fused: the results of
    FRP_NO_BLOCK_FUSE=1; the first call, the capturing call and three replays return the same bits and charge the same counters."""
    engine = fresh_engine
    rng = np.random.default_rng(43)
    raw, blob = get_raw_and_blob((1, 1, 1, 1), (2, 1, 1, 1))
    B, H, W, K = 3, 256, 384, 5
    engine.load_weights(blob)
    engine.gallery_set(rng.standard_normal((300, 512)).astype(np.float32))
    engine.upload_frames(_frames(rng, B, H, W))
    probe = engine.detect_resident((H, W), max_faces=64, det_thresh=1e-6, nms_iou=0.4)
    thr = float(np.clip(np.median(np.sort(probe["scores"], axis=1)[:, ::-1][:, 2]), 1e-4, 0.9999))      # ~3 faces per frame survive
    keys = ("boxes", "kps", "scores", "counts", "emb", "match_idx", "match_cos")
    ckeys = ("det_conv_flops", "det_conv_launches", "emb_conv_flops", "emb_conv_launches")

    def run():
        engine.reset_counters()
        engine.process_resident(K, det_thresh=thr, flags=0)
        r = engine.fetch_results()
        c = engine.counters()
        return r, {k: c[k] for k in ckeys}

    monkeypatch.setenv("FRP_BLOCK_FUSE_ALL", "1")
    replays0 = engine.graph_replays()
    first, c_first = run()
    assert 0 < first["counts"].sum() < B * K
    for i in range(4):
        got, c_got = run()
        for k in keys:
            assert np.array_equal(first[k], got[k]), f"call {i + 2}: {k} differs from the first call"
        assert c_got == c_first
    assert engine.graph_replays() - replays0 >= 2 * 3
    monkeypatch.delenv("FRP_BLOCK_FUSE_ALL")
    monkeypatch.setenv("FRP_NO_BLOCK_FUSE", "1")
    sep, c_sep = run()
    for k in keys:
        assert np.array_equal(first[k], sep[k]), k
    assert c_first["det_conv_launches"] == c_sep["det_conv_launches"] - 1 and c_first["emb_conv_launches"] == c_sep["emb_conv_launches"] - 1
    assert c_first["det_conv_flops"] == c_sep["det_conv_flops"] and c_first["emb_conv_flops"] == c_sep["emb_conv_flops"]
