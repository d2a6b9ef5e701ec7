"""Inputs of the embedder tail's parity tests (tests/test_gpu_embed_tail_exact.py; their conditions: tests/test_embed_tail_inputs.py).
Generators are cached and their arrays read-only; nothing device-specific is imported: the lists are functions of the CU count.

A shape is (K, D, n, cap, modes): x [cap, K] fp16 of which n rows exist, w [D, K] fp16, bias [D] fp32; a mode is "host", "device", "none"
or a forced factor s >= 2 (Engine.debug_fc_l2norm).  K must be a multiple of 64 and a split needs nk = K / 64 >= 64:
    K = 4096   nk 64: factors 2, 4, 8            the smallest K that splits
    K = 6400   nk 100: factors 2, 4, 5, 10       a factor that is no power of two
    K = 25088  nk 392: the real FC, 49 below and 28 above 256 rows on 256 CUs - host and device mode only (25 MB of weights, 4 GFLOP)
    D = 512; 1024 (four elements per l2norm thread, eight cout tiles); 96 (idle l2norm lanes, one ragged cout tile)
    n / cap    1/1, 3/3, 3/64, 0/8 (no row may be written), 255/320, 256/320, 257/320, 320/320, and the row counts either side of every
               step of pick_ksplit for the CU count in use (K = 4096 and 6400 reach theirs with D = 1024, at 1024/1025 and 768/769 rows
               on 256 CUs).
In EVERY case the rows of x at or beyond n hold NaNs and infinities: no kernel may read them.

exact      x in {-2 .. 2}, w in {-1, 0, 1} with 200 / K of the weights non-zero, integer bias in {-3 .. 3}: v has a standard deviation of
           20, |v| <= 150, every partial sum in any order and any split is an integer below 2^24 and so is ss (D * max v^2 < 2^24).  Row
           n - 1 (n >= 3) is a zero row of x: v = bias.
probes     one-hot rows: row 2 j has its 1 at the first k of slice j of factor s, row 2 j + 1 at the last; w[c, k] holds the base-64 digits
           of k (c % 3 == 0: k % 64, 1: (k / 64) % 64, 2: k / 4096 + 1), the bias (c % 5) - 2: v = digits + bias names the k a row saw and
           is no multiple of the digits alone, so a slice summed twice shows behind the normalisation.  Exact like the exact family.
general    standard-normal x and w / sqrt(K), rounded once to fp16, bias 0.25 * normal in fp32, held to embed_tail_model.bound.  Besides
           the ordinary rows (where a case has room: n >= 3 for the first, n >= 16 for all of them):
             edge rows, one per factor the case's modes can take: zeros but for the last 64-wide k-step of slice 0, the first of slice
                       1 and the last of the last slice.  A k-range that is off by one step, a missing bias or a missing slab is a few
                       per cent of an ordinary row of K = 25088 - below what K additions may cost there - but most of an edge row
             a zero row of x (v = bias: the bias alone, to a few ulps)
             a row with an infinity (at a k where every weight is non-zero) and a row with a NaN: both come out NaN throughout
           One case has a zero bias and a zero row: exact zeros.
"""
import functools

import numpy as np

import embed_tail_model as tm

N_CAP = [(1, 1), (3, 3), (3, 64), (0, 8), (255, 320), (256, 320), (257, 320), (320, 320)]
FORCED = {4096: (2, 4, 8), 6400: (2, 4, 5, 10)}
TILE_FLAGS = (0, 1 << 17, 1 << 18)          # frp_conv2d_nhwc's tile-class bits: conv_pick's choice, quarter tiles, 256-pixel tiles
K_REAL = 25088


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def _all_modes(K):
    return ("host", "device", "none") + FORCED[K]


def _round_cap(n):
    return (n + 63) // 64 * 64 + 64


@functools.lru_cache(maxsize=None)
def shapes(n_cu=256):
    """[(K, D, n, cap, modes)]"""
    out = []
    for n, cap in N_CAP:
        out.append((4096, 512, n, cap, _all_modes(4096)))
    for n, cap in ((3, 64), (257, 320)):
        out.append((4096, 1024, n, cap, _all_modes(4096)))
        out.append((4096, 96, n, cap, _all_modes(4096)))
    for n, cap in ((3, 64), (255, 320), (256, 320), (257, 320)):
        out.append((6400, 512, n, cap, _all_modes(6400)))
    for n, cap in ((3, 64), (256, 320), (257, 320), (320, 320)):
        out.append((K_REAL, 512, n, cap, ("host", "device")))
    # both sides of every factor step for this CU count
    for K, D, reach in ((4096, 1024, 1280), (6400, 1024, 1280), (K_REAL, 512, 320)):
        for lo, hi in tm.factor_steps(D, K, n_cu, reach)[:2]:
            for n in (lo, hi):
                out.append((K, D, n, min(_round_cap(hi), max(reach, hi)), ("host", "device")))
    seen, uniq = set(), []
    for s in out:
        if s[:4] not in seen:
            seen.add(s[:4])
            uniq.append(s)
    return tuple(uniq)


def case_id(shape):
    K, D, n, cap = shape[:4]
    return f"K{K}-D{D}-n{n}of{cap}"


def mode_factor(mode, K, D, n, n_cu):
    """the factor both kernels use in `mode` (1: no split)"""
    if mode in ("host", "device"):
        return tm.pick_ksplit(n, D, K, n_cu)
    return 1 if mode == "none" else int(mode)


def case_factors(shape, n_cu):
    """the factors > 1 a case's modes take, and the one its capacity would"""
    K, D, n, cap, modes = shape
    f = [mode_factor(m, K, D, n, n_cu) for m in modes] + [tm.pick_ksplit(cap, D, K, n_cu)]
    return tuple(sorted({s for s in f if s > 1}, reverse=True))


def _poison(x, n):
    """rows at or beyond n: NaNs and infinities"""
    x[n:] = np.float16(np.nan)
    x[n:, 1::2] = np.float16(np.inf)
    x[n:, 2::4] = np.float16(-np.inf)


# ---------------------------------------------------------------------------------------------------- exact family
@functools.lru_cache(maxsize=None)
def exact_weights(K, D):
    rng = np.random.default_rng([7, K, D])
    w = rng.choice([-1, 1], size=(D, K)) * (rng.random((D, K)) < 200.0 / K)
    return _ro(w.astype(np.float16), rng.integers(-3, 4, size=D).astype(np.float32))


@functools.lru_cache(maxsize=4)
def exact_case(K, D, n, cap):
    """-> (x16 [cap, K], w16 [D, K], bias [D], v [n, D] int64)"""
    w16, bias = exact_weights(K, D)
    rng = np.random.default_rng([8, K, D, n, cap])
    xi = rng.integers(-2, 3, size=(cap, K))
    if n >= 3:
        xi[n - 1] = 0
    x16 = xi.astype(np.float16)
    _poison(x16, n)
    v = (xi[:n].astype(np.float64) @ w16.astype(np.float64).T + bias).astype(np.int64)
    return _ro(x16, w16, bias, v)


# ---------------------------------------------------------------------------------------------------- slice probes
@functools.lru_cache(maxsize=None)
def probe_weights(K, D):
    k, c = np.arange(K)[None, :], np.arange(D)[:, None]
    w = np.where(c % 3 == 0, k % 64, np.where(c % 3 == 1, (k // 64) % 64, k // 4096 + 1))
    return _ro(w.astype(np.float16), ((np.arange(D) % 5) - 2).astype(np.float32))


def probe_ks(K, s):
    """the k of probe row j = 0 .. 2 s - 1: first and last k of every slice of factor s"""
    per = K // s
    return np.array([(j // 2) * per + (0 if j % 2 == 0 else per - 1) for j in range(2 * s)])


@functools.lru_cache(maxsize=4)
def probe_case(K, D, s, n):
    """-> (x16 [n, K], w16, bias, v [n, D] int64); n >= 2 s, the rows behind the probes are zero rows (v = bias)"""
    assert n >= 2 * s and K % (64 * s) == 0
    w16, bias = probe_weights(K, D)
    x16 = np.zeros((n, K), np.float16)
    ks = probe_ks(K, s)
    x16[np.arange(2 * s), ks] = 1
    v = np.tile(bias.astype(np.int64), (n, 1))
    v[:2 * s] += w16[:, ks].T.astype(np.int64)
    return _ro(x16, w16, bias, v)


def probe_rows_for(K, D, s, n_cu):
    """the smallest row count n >= 2 s at which the host's rule takes factor s, or None (the probe is then forced)"""
    for n in range(2 * s, 1281):
        if tm.pick_ksplit(n, D, K, n_cu) == s:
            return n
    return None


# ---------------------------------------------------------------------------------------------------- general family
@functools.lru_cache(maxsize=None)
def general_weights(K, D):
    rng = np.random.default_rng([9, K, D])
    w16 = (rng.standard_normal((D, K), np.float32) / np.float32(np.sqrt(K))).astype(np.float16)
    return _ro(w16, (0.25 * rng.standard_normal(D)).astype(np.float32))


ORDINARY, EDGE, ZERO, HAS_INF, HAS_NAN = range(5)


@functools.lru_cache(maxsize=4)
def general_case(K, D, n, cap, factors=(), zero_bias=False):
    """-> (x16 [cap, K], w16, bias, kind [n]); factors: one edge row each"""
    w16, bias = general_weights(K, D)
    if zero_bias:
        bias = _ro(np.zeros(D, np.float32))
    rng = np.random.default_rng([10, K, D, n, cap])
    x = rng.standard_normal((cap, K), np.float32)
    kind = np.full(n, ORDINARY)
    edges = factors if n >= 16 else factors[:1] if n >= 3 else ()
    for j, s in enumerate(edges):
        per = K // s
        keep = np.r_[per - 64:per + 64, K - 64:K]
        vals = x[1 + j, keep].copy()
        x[1 + j] = 0
        x[1 + j, keep] = vals
        kind[1 + j] = EDGE
    x16 = x.astype(np.float16)
    if n >= 16:
        k_inf = int(np.nonzero((w16 != 0).all(0))[0][0])
        x16[n // 2, k_inf] = np.float16(np.inf)
        x16[n // 2 + 2, 5] = np.float16(np.nan)
        x16[n - 2] = 0
        kind[[n // 2, n // 2 + 2, n - 2]] = HAS_INF, HAS_NAN, ZERO
    elif zero_bias and n >= 2:
        x16[n - 1] = 0
        kind[n - 1] = ZERO
    _poison(x16, n)
    return _ro(x16, w16, bias, kind)


ZERO_BIAS_SHAPE = (4096, 512, 3, 64, ("host", "device", "none", 8))
