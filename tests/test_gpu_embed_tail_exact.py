"""The embedder's tail on the device - the split-K FC (csrc/conv_mfma.hip, the `p.ksplit > 1` branch) and l2norm_kernel
(csrc/aux_kernels.hip), launched by frp_debug_fc_l2norm exactly as a pass launches them - held to the float64 reference of
tests/embed_tail_model.py: the exact family and the slice probes to the bit, the general family to the derived bound, device-count
against host-count mode bit for bit, the 0xFF fill behind the rows that exist.  The inputs and the conditions these assertions rest on:
tests/embed_tail_cases.py, tests/test_embed_tail_inputs.py (no device).  Nothing here compares the device with itself but the mode
comparisons, and those come on top of the reference.

Measured on an MI355X (256 CUs), largest err / bound of the general family over all cases and modes: emb 1.2e-4, emb16 0.54
(the fp16 rounding is most of the emb16 bound; K additions in the worst order are most of the emb bound and a random walk stays far
inside it); the exact family and the probes held to the bit in every mode and tile class."""
import numpy as np
import pytest

from frp_amd.native import FrpError

import embed_tail_cases as tc
import embed_tail_model as tm

pytestmark = pytest.mark.gpu

SHAPES = tc.shapes(256)
IDS = [tc.case_id(s) for s in SHAPES]
_RUNS = {}


@pytest.fixture(scope="module")
def n_cu(engine):
    return engine.debug_fc_l2norm(np.zeros((1, 64), np.float16), np.zeros((8, 64), np.float16), np.zeros(8, np.float32), 1)[2]


def _run(engine, family, shape, mode, flags, n_cu):
    """one launch of the tail on a case (host and device mode are kept: the mode comparisons reuse what the reference tests ran)"""
    K, D, n, cap = shape[:4]
    key = (family, K, D, n, cap, mode, flags)
    res = _RUNS.get(key)
    if res is None:
        if family == "exact":
            x16, w16, bias, _ = tc.exact_case(K, D, n, cap)
        else:
            x16, w16, bias, _ = tc.general_case(K, D, n, cap, tc.case_factors(shape, n_cu), family == "zero-bias")
        emb, emb16, ncu, factor = engine.debug_fc_l2norm(x16, w16, bias, n, mode, flags)
        assert ncu == n_cu and factor == tm.pick_ksplit(n, D, K, n_cu), (ncu, factor)            # the reported factor is the model's
        assert tm.is_fill(emb[n:]).all() and tm.is_fill(emb16[n:]).all(), f"{mode}: a row at or beyond n = {n} was written"
        res = (emb, emb16)
        if flags == 0 and mode in ("host", "device"):
            _RUNS[key] = res
    return res


def _device_step_shapes(n_cu):
    """the shapes either side of this device's factor steps that the fixed list (computed for 256 CUs) does not hold"""
    have = {s[:4] for s in SHAPES}
    return [s for s in tc.shapes(n_cu) if s[:4] not in have]


# ---------------------------------------------------------------------------------------------------- exact family
def _check_exact(engine, shape, n_cu):
    K, D, n, cap, modes = shape
    v = tc.exact_case(K, D, n, cap)[3]
    want32, want16 = tm.exact_bits(v) if n else (np.zeros((0, D), np.float32), np.zeros((0, D), np.float16))
    for mode in modes:
        for flags in tc.TILE_FLAGS:
            emb, emb16 = _run(engine, "exact", shape, mode, flags, n_cu)
            what = f"{tc.case_id(shape)} mode {mode} (factor {tc.mode_factor(mode, K, D, n, n_cu)}) flags {flags:#x}"
            if not tm.same_bits(emb[:n], want32):                    # (how far off, for the report: the bound of exact operands is term C alone)
                err = np.abs(emb[:n].astype(np.float64) - tm.normalize(v))
                pytest.fail(f"{what}: emb differs from the exact bits in {int((emb[:n] != want32).sum())} elements, largest error {err.max():.3e}")
            assert tm.same_bits(emb16[:n], want16), f"{what}: emb16"


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exact_family_to_the_bit_in_every_mode_and_tile_class(engine, n_cu, shape):
    _check_exact(engine, shape, n_cu)


# ---------------------------------------------------------------------------------------------------- slice probes
PROBES = [(4096, 512, 2), (4096, 512, 4), (4096, 512, 8), (6400, 512, 2), (6400, 512, 4), (6400, 512, 5), (6400, 512, 10), (4096, 96, 8),
          (4096, 1024, 4), (tc.K_REAL, 512, "below"), (tc.K_REAL, 512, "above")]


@pytest.mark.parametrize("K,D,s", PROBES, ids=[f"K{K}-D{D}-s{s}" for K, D, s in PROBES])
def test_slice_probes_every_slice_covers_its_k_range_once(engine, n_cu, K, D, s):
    runs = []
    if isinstance(s, str):                    # the real FC: the factor this device takes below / above its first step, in host and device mode
        steps = tm.factor_steps(D, K, n_cu, 1280)
        s = tm.pick_ksplit(steps[0][0] if s == "below" else steps[0][1], D, K, n_cu) if steps else tm.pick_ksplit(1, D, K, n_cu)
        n = tc.probe_rows_for(K, D, s, n_cu) if s > 1 else None
        runs = [(n, "host"), (n, "device")] if n else []
    if not runs:
        s = max(s, 2)
        while (K // 64) % s:
            s += 1
        runs = [(2 * s, s)]                   # a forced factor
    for n, mode in runs:
        x16, w16, bias, v = tc.probe_case(K, D, s, n)
        want32, want16 = tm.exact_bits(v)
        emb, emb16, _, factor = engine.debug_fc_l2norm(x16, w16, bias, n, mode)
        assert mode not in ("host", "device") or factor == s
        bad = np.nonzero((emb.view(np.uint32) != want32.view(np.uint32)).any(1))[0]
        ks = tc.probe_ks(K, s)
        assert bad.size == 0, (f"factor {s} mode {mode}: rows {bad[:8].tolist()} differ - probe row j sits at k = " +
                               f"{[int(ks[j]) if j < 2 * s else None for j in bad[:8]]} (slice j / 2, first / last k)")
        assert tm.same_bits(emb16, want16)


# ---------------------------------------------------------------------------------------------------- general family
def _check_general(engine, shape, n_cu, family="general"):
    K, D, n, cap, modes = shape
    x16, w16, bias, kind = tc.general_case(K, D, n, cap, tc.case_factors(shape, n_cu), family == "zero-bias")
    fin = ~np.isin(kind, [tc.HAS_INF, tc.HAS_NAN])
    worst = {"emb": 0.0, "emb16": 0.0}
    bounds = {}
    for mode in modes:
        ks = tc.mode_factor(mode, K, D, n, n_cu)
        emb, emb16 = _run(engine, family, shape, mode, 0, n_cu)
        if n == 0:
            continue
        if ks not in bounds:
            bounds[ks] = tm.bound(x16, w16, bias, n, ks)
        ref, b32, b16, dom = bounds[ks]
        assert dom[fin].all()
        assert np.isnan(emb[:n][~fin]).all() and np.isnan(emb16[:n][~fin].astype(np.float32)).all(), f"mode {mode}: an inf / NaN row must be NaN throughout"
        for name, got, b in (("emb", emb, b32), ("emb16", emb16, b16)):
            ok, ratio = tm.within(got[:n][fin], ref[fin], b[fin])
            worst[name] = max(worst[name], ratio)
            assert ok, f"{tc.case_id(shape)} mode {mode} (factor {ks}) {name}: largest err / bound {ratio:.4f}"
        if family == "zero-bias":
            z = kind == tc.ZERO
            assert z.sum() == 1 and not emb[:n][z].any() and not emb16[:n][z].any() and not np.signbit(emb[:n][z]).any()
    factors = sorted({tc.mode_factor(m, K, D, n, n_cu) for m in modes})
    print(f"embed-tail general {tc.case_id(shape)}: factors {factors}, largest err / bound emb {worst['emb']:.2e} emb16 {worst['emb16']:.4f}")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("shape", SHAPES + (tc.ZERO_BIAS_SHAPE,), ids=IDS + ["zero-bias"])
def test_general_family_within_the_derived_bound(engine, n_cu, shape):
    _check_general(engine, shape, n_cu, "zero-bias" if shape is tc.ZERO_BIAS_SHAPE else "general")


# ---------------------------------------------------------------------------------------------------- device count against host count
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_device_count_equals_host_count_bit_for_bit(engine, n_cu, shape):
    n = shape[2]
    for family in ("exact", "general"):
        host, dev = _run(engine, family, shape, "host", 0, n_cu), _run(engine, family, shape, "device", 0, n_cu)
        assert tm.same_bits(dev[0], host[0]) and tm.same_bits(dev[1], host[1]), f"{tc.case_id(shape)} {family}: rows below n = {n} or the fill differ"
        if n == 0:
            assert tm.is_fill(dev[0]).all() and tm.is_fill(host[0]).all() and tm.is_fill(dev[1]).all() and tm.is_fill(host[1]).all()


def test_factor_steps_of_this_device(engine, n_cu):
    """the row counts either side of pick_ksplit's steps for the CU count the handle reports (on 256 CUs the fixed list holds them)"""
    for shape in _device_step_shapes(n_cu):
        _check_exact(engine, shape, n_cu)
        _check_general(engine, shape, n_cu)
        for family in ("exact", "general"):
            host, dev = _run(engine, family, shape, "host", 0, n_cu), _run(engine, family, shape, "device", 0, n_cu)
            assert tm.same_bits(dev[0], host[0]) and tm.same_bits(dev[1], host[1]), tc.case_id(shape)
    for K, D, reach in ((4096, 1024, 1280), (6400, 1024, 1280), (tc.K_REAL, 512, 320)):
        have = {s[2] for s in SHAPES + tuple(_device_step_shapes(n_cu)) if s[0] == K and s[1] == D}
        for lo, hi in tm.factor_steps(D, K, n_cu, reach)[:2]:
            assert lo in have and hi in have


# ---------------------------------------------------------------------------------------------------- poison
@pytest.mark.parametrize("K,D,n,cap", [(4096, 512, 3, 64), (4096, 96, 257, 320), (6400, 512, 255, 320), (tc.K_REAL, 512, 3, 64), (4096, 512, 0, 8)])
def test_rows_behind_n_are_neither_read_nor_written(engine, n_cu, K, D, n, cap):
    shape = next(s for s in SHAPES if s[:4] == (K, D, n, cap))
    x16, w16, bias, _ = tc.general_case(K, D, n, cap, tc.case_factors(shape, n_cu))
    assert not np.isfinite(x16[n:].astype(np.float32)).any()
    clean = np.array(x16)
    clean[n:] = 0
    for mode in ("device", "host"):
        want = _run(engine, "general", shape, mode, 0, n_cu)                                     # x rows at or beyond n: NaNs and infinities
        got = engine.debug_fc_l2norm(clean, w16, bias, n, mode)[:2]                              # ... zeros
        assert tm.same_bits(got[0], want[0]) and tm.same_bits(got[1], want[1]), f"mode {mode}: the rows of x behind n reach the rows below n"
        assert tm.is_fill(got[0][n:]).all() and tm.is_fill(got[1][n:]).all()


# ---------------------------------------------------------------------------------------------------- refusals
def _refused(fn):
    with pytest.raises(FrpError) as e:
        fn()
    assert e.value.code == -1 and str(e.value).split(":", 1)[1].strip()          # FRP_ERR_INVALID and the library's message
    return e.value


def test_refusals(engine, n_cu):
    x, w, b = np.ones((8, 4096), np.float16), np.ones((512, 4096), np.float16), np.zeros(512, np.float32)
    _refused(lambda: engine.debug_fc_l2norm(x, w, b, 8, 3))                      # 3 does not divide nk = 64
    _refused(lambda: engine.debug_fc_l2norm(x, w, b, 8, 128))                    # 128 does not divide 64 either
    _refused(lambda: engine.debug_fc_l2norm(x, w, b, 9))                         # n > cap
    _refused(lambda: engine.debug_fc_l2norm(x, w, b, -1))
    _refused(lambda: engine.debug_fc_l2norm(x, w, b, 8, -2))                     # no such mode
    _refused(lambda: engine.debug_fc_l2norm(x, w, b, 8, "host", 1 << 8))         # a flag that is no tile-class bit
    _refused(lambda: engine.debug_fc_l2norm(x[:, :64], np.ones((1032, 64), np.float16), np.zeros(1032, np.float32), 8))      # D > 1024
    _refused(lambda: engine.debug_fc_l2norm(np.ones((8, 4104), np.float16), np.ones((512, 4104), np.float16), b, 8, 2))      # a split of a ragged K
    emb, emb16, ncu, factor = engine.debug_fc_l2norm(x, w, b, 8, 2)              # the handle is as good as before
    assert ncu == n_cu and np.array_equal(emb, np.full((8, 512), np.float32(1.0) / np.sqrt(np.float32(512.0)), np.float32))
