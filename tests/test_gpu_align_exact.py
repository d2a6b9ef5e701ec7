"""GPU tests of face alignment (align_kernel, csrc/aux_kernels.hip) against the float64 reference of tests/align_model.py.

exact family    landmarks s * template + T with s in {1, 2, 1/2}: every source coordinate and every weight (0, 1/4, 1/2, 1) is exact in
                fp32, so the chips equal the reference rounded to fp16, value for value.
general family  rotated / scaled / jittered landmarks: |chips - blob| <= tol on every pixel and channel, tol derived in align_model
                (fp32 source coordinates times the local slope + fp32 accumulation + the fp16 rounding); no pixel is excluded.
pipeline launch Engine.align_resident: run_faces' own launch (compacted face list, frame of each slot, frame stride, count on the host
                or on the device) against the stand-alone call and the reference of the right frame.
tests/test_align_inputs.py shows on the host that fp32 arithmetic meets these assertions on these inputs and that a shifted tap, swapped
channels or weights and a replicated border do not.  Largest err / tol measured on the device: DESIGN.md."""
import numpy as np
import pytest

import align_cases as ac
import align_model as am
from frp_amd.native import FLAG_RGB, FrpError

pytestmark = pytest.mark.gpu

MINUS_ONE, FILL = 0xBC00, 0xFFFF


def _pad_lanes_are_zero(chips):
    return bool(np.all(chips[..., 3:].view(np.uint16) == 0))


# ------------------------------------------------------------------------------------------------ (a) exact family
@pytest.mark.parametrize("case", ac.EXACT_CASES, ids=ac.exact_id)
def test_exact_family(engine, case):
    s, T, (H, W) = case
    kps = ac.exact_kps64(s, T).astype(np.float32)
    frame = ac.noise(H, W)
    want = am.reference(frame, kps)[0].astype(np.float16)
    chips = engine.align(frame, kps[None])
    assert chips.shape == (1, 112, 112, 8)
    assert np.array_equal(chips[0, ..., :3], want)
    assert _pad_lanes_are_zero(chips)
    rgb = engine.align(np.ascontiguousarray(frame[..., ::-1]), kps[None], flags=FLAG_RGB)
    assert np.array_equal(rgb.view(np.uint16), chips.view(np.uint16))


# ------------------------------------------------------------------------------------------------ (b) general family
@pytest.mark.parametrize("name,kind,rgb", ac.GENERAL_RUNS)
def test_general_family(engine, name, kind, rgb):
    (H, W), kps = ac.GENERAL_CASES[name]
    frame = ac.frame(kind, H, W)
    chips = engine.align(frame, kps, flags=FLAG_RGB if rgb else 0)
    assert _pad_lanes_are_zero(chips)
    for i, k in enumerate(kps):
        blob, tol = am.reference(frame, k, rgb=rgb)
        print(f"align {name} {kind} rgb={int(rgb)} face {i}: err/tol {am.worst(chips[i, ..., :3], blob, tol):.3f}")
        assert am.within(chips[i, ..., :3], blob, tol), (i, am.worst(chips[i, ..., :3], blob, tol))


# ------------------------------------------------------------------------------------------------ (c) the pipeline's launch
@pytest.mark.parametrize("device_count", [False, True])
def test_pipeline_launch(engine, device_count):
    frames, kps, exact = ac.pipeline_case()
    slots = ac.pipeline_slots()
    n = len(slots)
    engine.upload_frames(frames)
    chips = engine.align_resident(kps, ac.PIPE_COUNTS, device_count=device_count)
    assert chips.shape == (ac.PIPE_B * ac.PIPE_K, 112, 112, 8)
    assert np.all(chips[n:].view(np.uint16) == FILL)                # only sum(counts) chips are written, whatever the launch was sized for
    assert _pad_lanes_are_zero(chips[:n])
    for i, (b, k) in enumerate(slots):
        got = chips[i, ..., :3]
        blob, tol = am.reference(frames[b], kps[b, k])
        print(f"align_resident device_count={int(device_count)} chip {i} = frame {b} face {k}: err/tol {am.worst(got, blob, tol):.3f}")
        if exact[b, k]:
            assert np.array_equal(got, blob.astype(np.float16))
        assert am.within(got, blob, tol)
        for other in range(ac.PIPE_B):                              # the same warp of another frame's pixels is not accepted
            if other != b:
                wblob, wtol = am.reference(frames[other], kps[b, k])
                assert not am.within(got, wblob, wtol)
    # the channel flag reaches this launch too
    engine.upload_frames(np.ascontiguousarray(frames[..., ::-1]))
    rgb = engine.align_resident(kps, ac.PIPE_COUNTS, flags=FLAG_RGB, device_count=device_count)
    assert np.array_equal(rgb.view(np.uint16), chips.view(np.uint16))
    # and it computes what the stand-alone entry point computes, bit for bit
    for i, (b, k) in enumerate(slots):
        alone = engine.align(frames[b], kps[b, k][None])
        assert np.array_equal(alone[0].view(np.uint16), chips[i].view(np.uint16))


@pytest.mark.parametrize("device_count", [False, True])
def test_pipeline_launch_without_faces(engine, device_count):
    frames, kps, _ = ac.pipeline_case()
    engine.upload_frames(frames)
    chips = engine.align_resident(kps, np.zeros(ac.PIPE_B, np.int32), device_count=device_count)
    assert np.all(chips.view(np.uint16) == FILL)


# ------------------------------------------------------------------------------------------------ (d) landmarks without a transform
def test_landmarks_without_a_transform(engine):
    """degenerate, NaN, inf and huge landmarks between valid faces: their chips are the border value (-1, -1, -1, 0...) exactly and the
    neighbours are untouched.  (The source coordinates are clamped in float before they become integers and every address is clamped
    again: csrc/aux_kernels.hip.)"""
    (H, W), valid = ac.GENERAL_CASES["240x320_four_faces"]
    frame = ac.noise(H, W)
    bad = ac.degenerate_sets()
    kps, is_bad = [valid[0]], [False]
    for j, k in enumerate(bad.values()):
        kps += [k, valid[(j + 1) % len(valid)]]
        is_bad += [True, False]
    kps = np.array(kps, np.float32)
    chips = engine.align(frame, kps)
    assert _pad_lanes_are_zero(chips)
    names = iter(bad)
    for i in range(len(kps)):
        if is_bad[i]:
            assert np.all(chips[i, ..., :3].view(np.uint16) == MINUS_ONE), next(names)
        else:
            blob, tol = am.reference(frame, kps[i])
            assert am.within(chips[i, ..., :3], blob, tol), (i, am.worst(chips[i, ..., :3], blob, tol))


# ------------------------------------------------------------------------------------------------ (e) refusals
def test_refusals(engine):
    kps = ac.exact_kps64(1.0, (0, 0)).astype(np.float32)
    with pytest.raises(FrpError):
        engine.align(np.zeros((5, 2, 3), np.uint8), kps[None])                  # W = 2: a row is shorter than one 8-byte read
    with pytest.raises(FrpError):
        engine.align(ac.noise(40, 50), np.zeros((0, 5, 2), np.float32))         # M = 0
    engine.upload_frames(np.zeros((1, 5, 2, 3), np.uint8))
    with pytest.raises(FrpError):
        engine.align_resident(kps[None, None], [1])
    with pytest.raises(FrpError):
        engine.align_resident(kps[None, None], [2])                             # a count beyond max_faces
    chips = engine.align(ac.noise(40, 50), kps[None])                           # the handle is still usable
    assert np.array_equal(chips[0, ..., :3], am.reference(ac.noise(40, 50), kps)[0].astype(np.float16))
