"""Host tests of the alignment inputs (tests/align_cases.py): each GPU case of tests/test_gpu_align_exact.py is one where fp32 arithmetic
can meet what the GPU test asserts - shown with the fp32 transcription of the kernel (align_model.kernel_fp32_model, with and without
fused multiply-adds) - and the GPU assertion's predicate rejects a one-pixel shift, swapped channels, swapped weights and a replicated
border.  No GPU."""
import numpy as np
import pytest

import align_cases as ac
import align_model as am


def _model_both(frame, kps, rgb=False, mutant=None):
    return [am.kernel_fp32_model(frame, kps, rgb=rgb, fma=fma, mutant=mutant) for fma in (False, True)]


# ------------------------------------------------------------------------------------------------ exact family
@pytest.mark.parametrize("case", ac.EXACT_CASES, ids=ac.exact_id)
def test_exact_case_is_exact_in_fp32(case):
    s, T, (H, W) = case
    kps64 = ac.exact_kps64(s, T)
    assert np.array_equal(kps64, kps64.astype(np.float32).astype(np.float64))          # the landmarks are float32 numbers
    kps = kps64.astype(np.float32)
    frame = ac.noise(H, W)
    want = am.reference(frame, kps)[0].astype(np.float16)
    for got in _model_both(frame, kps):
        assert np.array_equal(got, want)
    # the RGB flag on the channel-reversed frame is the same computation
    rev = np.ascontiguousarray(frame[..., ::-1])
    assert np.array_equal(am.reference(rev, kps, rgb=True)[0], am.reference(frame, kps)[0])
    for got in _model_both(rev, kps, rgb=True):
        assert np.array_equal(got, want)
    # the reference really is the intended warp: source point (s u + Tx, s v + Ty)
    Ai = am._inverse(am.similarity(kps))
    assert np.abs(Ai - np.array([[s, 0, T[0]], [0, s, T[1]]])).max() < 1e-10


def test_exact_values_survive_the_double_rounding():
    """every value an exact case can produce - products of weights 0, 1/4, 1/2, 1 with u8 taps: k/4, k = 0..1020 - normalised in fp32 as the
    kernel does and then rounded to fp16 equals the float64 value rounded once"""
    x = np.arange(1021, dtype=np.float64) / 4
    f32 = np.float32
    k = ((x.astype(f32) - f32(127.5)) * f32(f32(1.0) / f32(127.5))).astype(f32).astype(np.float16)
    want = ((x - 127.5) / 127.5).astype(np.float16)
    assert np.array_equal(k.view(np.uint16), want.view(np.uint16))


def test_exact_cases_reach_the_clamped_loads():
    """what the table of cases claims about the kernel's branches: x0 = W-1 with the right tap outside (56x56, s = 0.5), every load clamped
    (1x3: bx_max = 1), most of the chip on the border (40x50, identity)"""
    u = np.arange(112)
    x0 = np.floor(0.5 * u).astype(int)
    assert (x0 == 55).any() and (x0 + 1 == 56).any()
    assert 3 * 3 - 8 == 1
    inside = (u[None, :] < 50) & (u[:, None] < 40)
    assert inside.mean() < 1 / 3


# ------------------------------------------------------------------------------------------------ general family
@pytest.mark.parametrize("name,kind,rgb", ac.GENERAL_RUNS)
def test_general_case_meets_the_bound_in_fp32(name, kind, rgb):
    (H, W), kps = ac.GENERAL_CASES[name]
    frame = ac.frame(kind, H, W)
    for i, k in enumerate(kps):
        blob, tol = am.reference(frame, k, rgb=rgb)
        for got in _model_both(frame, k, rgb=rgb):
            assert am.within(got, blob, tol), (i, am.worst(got, blob, tol))


def test_general_cases_cover_what_they_claim():
    """part of a chip outside the frame, source coordinates near 2000, a strong down- and up-scale; and every case has pixels inside"""
    def src(name, i):
        (H, W), kps = ac.GENERAL_CASES[name]
        Ai = am._inverse(am.similarity(kps[i]))
        v, u = np.mgrid[0:112, 0:112].astype(np.float64)
        sx, sy = Ai[0, 0] * u + Ai[0, 1] * v + Ai[0, 2], Ai[1, 0] * u + Ai[1, 1] * v + Ai[1, 2]
        return sx, sy, (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1), Ai
    for name, (_, kps) in ac.GENERAL_CASES.items():
        for i in range(len(kps)):
            assert src(name, i)[2].any(), (name, i)
    ins = src("240x320_four_faces", 3)[2]
    assert ins.any() and not ins.all()
    sx, _, ins, _ = src("64x2048_x_near_2000", 0)
    assert sx[ins].max() > 1990
    sx, sy, ins, _ = src("1088x1920_far_corner", 0)
    assert sx[ins].max() > 1900 and sy[ins].max() > 1070
    assert np.hypot(*src("33x47_down_and_up", 0)[3][:, 0]) < 0.4 and np.hypot(*src("33x47_down_and_up", 1)[3][:, 0]) > 3.5


# ------------------------------------------------------------------------------------------------ closed form
def _all_landmark_sets():
    sets = [ac.exact_kps64(s, T).astype(np.float32) for (s, T, _) in ac.EXACT_CASES]
    for _, kps in ac.GENERAL_CASES.values():
        sets += list(kps)
    sets += list(ac.pipeline_case()[1].reshape(-1, 5, 2))
    return sets


def test_closed_form_equals_umeyama():
    """the kernel's closed form and Umeyama's SVD with its reflection guard pick the same proper similarity: equal to 1e-12 of the
    matrix's largest entry on every landmark set of the tests, the mirrored one included"""
    for kps in _all_landmark_sets():
        M, ok = am.closed_form(kps)
        U = am.similarity(kps)
        assert ok
        assert np.abs(M - U).max() <= 1e-12 * np.abs(U).max(), np.abs(M - U).max()
        assert np.linalg.det(U[:, :2]) > 0
    # the mirrored set does take the guard: the unguarded cross-covariance has a negative determinant
    k = ac.GENERAL_CASES["240x320_mirrored"][1][0].astype(np.float64)
    t = am.TEMPLATE32.astype(np.float64)
    assert np.linalg.det((t - t.mean(0)).T @ (k - k.mean(0))) < 0
    # and a plainly mirrored template (x -> -x)
    km = am.TEMPLATE32 * np.array([-1, 1], np.float32)
    M, ok = am.closed_form(km)
    U = am.similarity(km)
    assert ok and np.abs(M - U).max() <= 1e-12 * np.abs(U).max() and np.linalg.det(U[:, :2]) > 0


def test_degenerate_sets_have_no_transform():
    for name, k in ac.degenerate_sets().items():
        assert not am.closed_form(k)[1], name
        for got in _model_both(ac.noise(240, 320), k):
            assert np.all(got.view(np.uint16) == 0xBC00), name


# ------------------------------------------------------------------------------------------------ mutants
def _fails_somewhere(mutate):
    """mutate(frame, kps, rgb) -> model output of a wrong kernel; True if the GPU predicate of some listed case rejects it"""
    for (s, T, (H, W)) in ac.EXACT_CASES:
        kps = ac.exact_kps64(s, T).astype(np.float32)
        frame = ac.noise(H, W)
        want = am.reference(frame, kps)[0].astype(np.float16)
        if not np.array_equal(mutate(frame, kps, False), want):
            return True
    for (name, kind, rgb) in ac.GENERAL_RUNS:
        (H, W), kps = ac.GENERAL_CASES[name]
        frame = ac.frame(kind, H, W)
        for k in kps:
            blob, tol = am.reference(frame, k, rgb=rgb)
            if not am.within(mutate(frame, k, rgb), blob, tol):
                return True
    return False


MUTANTS = {
    "rolled_x": lambda f, k, rgb: am.kernel_fp32_model(np.roll(f, 1, axis=1), k, rgb=rgb),
    "rolled_y": lambda f, k, rgb: am.kernel_fp32_model(np.roll(f, 1, axis=0), k, rgb=rgb),
    "r_b_swapped": lambda f, k, rgb: am.kernel_fp32_model(f, k, rgb=rgb)[..., ::-1],
    "ax_swapped": lambda f, k, rgb: am.kernel_fp32_model(f, k, rgb=rgb, mutant="swap_ax"),
    "replicate_border": lambda f, k, rgb: am.kernel_fp32_model(f, k, rgb=rgb, mutant="replicate"),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_rejected(name):
    assert _fails_somewhere(MUTANTS[name])


def test_unmutated_model_is_accepted():
    assert not _fails_somewhere(lambda f, k, rgb: am.kernel_fp32_model(f, k, rgb=rgb, fma=True))


@pytest.mark.parametrize("name", ["rolled_x", "rolled_y"])
def test_a_one_pixel_shift_breaks_the_bound_widely(name):
    """not one lucky pixel: on the noise frames a shifted tap breaks the bound on a third or more of the pixels that lie inside the image"""
    for case in ("240x320_four_faces", "1088x1920_far_corner"):
        (H, W), kps = ac.GENERAL_CASES[case]
        frame = ac.noise(H, W)
        blob, tol = am.reference(frame, kps[0])
        bad = np.abs(MUTANTS[name](frame, kps[0], False).astype(np.float64) - blob) > tol
        assert bad.any(-1).mean() > 0.33


# ------------------------------------------------------------------------------------------------ the pipeline case
def test_pipeline_frames_differ_enough():
    """a chip warped from another frame of the batch fails the predicate of its own frame, for every listed slot"""
    frames, kps, exact = ac.pipeline_case()
    for (b, k) in ac.pipeline_slots():
        blob, tol = am.reference(frames[b], kps[b, k])
        for other in range(ac.PIPE_B):
            if other == b:
                continue
            wrong = am.kernel_fp32_model(frames[other], kps[b, k])
            assert not am.within(wrong, blob, tol)
            assert not np.array_equal(wrong, blob.astype(np.float16))
        for got in _model_both(frames[b], kps[b, k]):
            if exact[b, k]:
                assert np.array_equal(got, blob.astype(np.float16))
            assert am.within(got, blob, tol)
    assert exact[0, 1] and exact[2, 2] and len(ac.pipeline_slots()) == 5
