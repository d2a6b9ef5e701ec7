"""native.Engine's pass-shape state on a stub library (no GPU, no libfrp.so): everything exists from __init__ on, one record holds the
(B, K) of the last pass, and an engine that has had no batch or pass reaches the library - whose refusal comes back as FrpError."""
import numpy as np
import pytest

from frp_amd import native


class StubLib:
    """stands in for the ctypes library: records every call's name and leading integer arguments; `refuse`: names that return -1"""

    def __init__(self, refuse=()):
        self.calls, self.refuse, self.host_alloc = [], set(refuse), 0

    def frp_create(self, device, cfg, handle):
        handle._obj.value = 1
        return 0

    def frp_destroy(self, h):
        pass

    def frp_last_error(self, h):
        return b"stub: refused"

    def frp_host_alloc(self, h, n):
        return self.host_alloc

    def frp_get_head_map(self, h, lv, out, nbytes, hl, wl):
        self.calls.append(("frp_get_head_map", lv, nbytes))
        hl._obj.value, wl._obj.value = 3, 4
        return -1 if "frp_get_head_map" in self.refuse else 0

    def __getattr__(self, name):
        if not name.startswith("frp_"):
            raise AttributeError(name)

        def call(h, *args):
            self.calls.append((name,) + tuple(a for a in args if isinstance(a, int)))
            return -1 if name in self.refuse else 0
        return call


@pytest.fixture()
def make_engine(monkeypatch):
    def make(refuse=()):
        lib = StubLib(refuse)
        monkeypatch.setattr(native, "load_library", lambda: lib)
        return native.Engine(0), lib
    return make


def test_a_fresh_engine_has_all_of_its_state_and_reaches_the_library(make_engine):
    eng, lib = make_engine(refuse=("frp_fetch_results", "frp_swap_frames", "frp_get_head_map", "frp_detect_resident", "frp_get_frames"))
    assert eng.resident_shape == (0, 0, 0) and eng._staged == (0, 0, 0) and eng._pass == (0, 0) and eng._det_batch == 0 and eng._yuv_keep == ()
    with pytest.raises(AttributeError):
        eng.resident_shape = (1, 2, 3)                                   # read-only
    for call in (eng.fetch_results, eng.swap_frames, eng.head_maps, lambda: eng.detect_resident((8, 8)), eng.get_frames, eng.fetch_within):
        lib.calls.clear()
        if call == eng.fetch_within:
            lib.refuse.add("frp_fetch_within")
        with pytest.raises(native.FrpError, match="stub: refused") as e:
            call()
        assert e.value.code == -1 and len(lib.calls) == 1                # the library was asked, once, and its answer surfaced
        if call == eng.fetch_results:
            assert lib.calls[0][:3] == ("frp_fetch_results", 0, 0)       # B = 0, K = 0
    assert eng.resident_shape == (0, 0, 0)                               # a refused swap changes nothing


def test_host_frames_with_a_failed_allocation_raises_the_librarys_error(make_engine):
    eng, lib = make_engine()
    with pytest.raises(native.FrpError, match="stub: refused") as e:
        eng.host_frames(2, 4, 4)
    assert e.value.code == -6                                            # FRP_ERR_OOM: what frp_host_alloc fails with


def test_every_pass_records_the_shape_it_used(make_engine):
    eng, lib = make_engine()
    frames = np.zeros((3, 8, 16, 3), np.uint8)
    eng.process_frames(frames, max_faces=5)
    assert eng._pass == (3, 5) and eng._det_batch == 3
    eng.upload_frames(frames[:2])
    assert eng.resident_shape == (2, 8, 16) and eng._pass == (3, 5)
    eng.process_resident(max_faces=7)
    assert eng._pass == (2, 7) and eng._det_batch == 3
    eng.process_pyramid_resident([(8, 16), (4, 8)], max_faces=6)
    assert eng._pass == (2, 6)
    lib.calls.clear()
    out = eng.fetch_results()
    assert lib.calls == [("frp_fetch_results", 2, 6)] and out["emb"].shape == (2, 6, 512)
    eng.set_within(0.5, 8)
    lib.calls.clear()
    idx, cos, n = eng.fetch_within()
    assert lib.calls == [("frp_fetch_within", 2, 6, 8)] and idx.shape == (2, 6, 8) and n.shape == (2, 6)
    # the detector-only calls move the head maps' batch and leave the fetchable pass alone
    det = eng.detect(frames, max_faces=4)
    assert eng._pass == (2, 6) and eng._det_batch == 3 and det["anchor_idx"].shape == (3, 4) and "emb" in det
    eng.upload_frames_async(frames[:1])
    assert eng.resident_shape == (2, 8, 16) and eng._staged == (1, 8, 16)
    eng.swap_frames()
    assert eng.resident_shape == (1, 8, 16)
    det = eng.detect_resident((4, 8), max_faces=9)
    assert eng._pass == (2, 6) and eng._det_batch == 1 and sorted(det) == ["anchor_idx", "boxes", "counts", "kps", "scores"]
    assert det["boxes"].shape == (1, 9, 4) and det["anchor_idx"].shape == (1, 9) and np.all(det["anchor_idx"] == -1)
    assert [a.shape for a in eng.head_maps()] == [(1, 3, 4, 32)] * 3
    z = np.zeros
    eng.finish_faces(z((1, 2, 4)), z((1, 2, 5, 2)), z((1, 2)), z(1), max_faces=2)
    assert eng._pass == (1, 2) and eng._det_batch == 1
    # a refused pass records nothing
    lib.refuse.add("frp_process_resident")
    with pytest.raises(native.FrpError):
        eng.process_resident(max_faces=11)
    assert eng._pass == (1, 2)


def test_the_pyramid_call_uploads_once_on_either_arm(make_engine):
    eng, lib = make_engine()
    frames = np.zeros((2, 8, 16, 3), np.uint8)
    for on_device in (True, False):
        lib.calls.clear()
        out = eng.process_frames_pyramid(frames, scales=(1.0, 0.5), max_faces=3, on_device=on_device)
        names = [c[0] for c in lib.calls]
        assert names.count("frp_upload_frames") == 1 and names[0] == "frp_upload_frames"
        assert names[1:] == (["frp_process_pyramid", "frp_fetch_results"] if on_device else ["frp_detect_resident"] * 2 + ["frp_finish_faces"])
        assert eng._pass == (2, 3) and out["emb"].shape == (2, 3, 512)
