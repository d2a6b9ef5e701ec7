"""Inputs of the matcher's parity tests (tests/test_gpu_match_exact.py; their conditions: tests/test_match_inputs.py).  Generators are
cached and their arrays read-only; nothing device-specific is imported.

exact family    integer rows with sum of squares exactly 1024 (64 entries of magnitude 3, 64 of 2, 192 of 1, 192 zeros): the unit row is
                x / 32, exact in fp16; sqrt(1024) and 1 / 32 are exact, every fp32 partial sum of squares is an integer < 2^24, so
                normalize_rows_kernel returns x / 32 whatever its summation order.  A score is an integer / 1024 and every partial sum
                of the products, in any order, is an integer multiple of 2^-10 of magnitude <= 1: exact in fp32.  The device must
                return the float64 reference's bits.
                Gallery rows keep their 64 threes, all positive, inside a fixed set P of 128 positions spread over the row (the other
                384 + 64 positions hold the +-2, +-1 and zeros at random): the `negative` query (-3 on half of P, -2 on the other half)
                then scores below -0.25 against EVERY row - the case where a masked or padded element that scored 0 would win.
general family  unit Gaussian rows rounded once to fp16 and handed over as fp16 (Engine.match_f16): held to match_model.score_bound.
normalisation   fp32 rows for normalize_rows_kernel (gallery_set + gallery_get): held to match_model.normalize_bound.
"""
import functools

import numpy as np

import match_model as mm

D = 512
EXACT_SHAPES = [(1, 1), (31, 5), (33, 32), (129, 33), (257, 64), (4097, 320), (70001, 512), (300, 513)]
GENERAL_SHAPES = [(1000, 33), (4097, 320), (70001, 512)]
ANCHOR = 7
Q_ANCHOR, Q_MINUS, Q_ZERO, Q_NEGATIVE = 0, 1, 2, 3          # query rows of every exact case with M >= 5 (M == 1: the negative query)

_P = np.sort(np.random.default_rng(1024).permutation(D)[:128])
_NOT_P = np.setdiff1d(np.arange(D), _P)
_REST = np.concatenate([np.full(64, 2), np.full(192, 1), np.zeros(192, np.int64)])


def _ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def exact_gallery_rows(rng, n):
    """n integer rows (float32), sum of squares 1024, the threes positive and inside P"""
    rows = np.zeros((n, D), np.int64)
    three = np.argsort(rng.random((n, 128)), axis=1)[:, :64]                     # 64 of P's 128 positions per row
    is3 = np.zeros((n, D), bool)
    is3[np.arange(n)[:, None], _P[three]] = True
    rows[is3] = 3
    rest = rng.permuted(np.tile(_REST, (n, 1)), axis=1) * rng.choice([-1, 1], size=(n, 448))
    rows[~is3] = rest.reshape(-1)
    return rows.astype(np.float32)


def exact_free_rows(rng, n):
    """n integer rows (float32), sum of squares 1024, magnitudes and signs anywhere"""
    base = np.concatenate([np.full(64, 3), _REST])
    return (rng.permuted(np.tile(base, (n, 1)), axis=1) * rng.choice([-1, 1], size=(n, D))).astype(np.float32)


def negative_query(rng):
    q = np.zeros(D, np.int64)
    p = rng.permutation(_P)
    q[p[:64]], q[p[64:]] = -3, -2
    q[rng.permutation(_NOT_P)[:192]] = rng.choice([-1, 1], size=192)
    return q.astype(np.float32)


def planted_rows(N):
    """rows that hold a copy of row ANCHOR: 7 + 4 (the other half-wave), 7 + 32 (another wave), N // 2 and N - 1 (another workgroup or
    round), wherever the gallery has room for them behind the anchor"""
    return sorted({r for r in (ANCHOR + 4, ANCHOR + 32, N // 2, N - 1) if ANCHOR < r < N})


@functools.lru_cache(maxsize=None)
def exact_case(N, M):
    """-> (G [N, 512] float32 integer rows, Q [M, 512] float32 integer rows (one of them zero)); the unit rows are G / 32, Q / 32"""
    rng = np.random.default_rng(100003 * N + M)
    G = exact_gallery_rows(rng, N)
    for r in planted_rows(N):
        G[r] = G[ANCHOR]
    neg = negative_query(rng)
    if M == 1:
        Q = neg[None].copy()
    else:
        assert M >= 5
        a = G[ANCHOR if N > ANCHOR else 0]
        Q = np.concatenate([a[None], -a[None], np.zeros((1, D), np.float32), neg[None], exact_free_rows(rng, M - 4)])
        if M > 40:
            Q[37] = G[N - 1]                                     # the last row of a ragged block, from a query of the second tile
    return _ro(G, Q)


def unit16(rows):
    """the exact family's unit rows as fp16: x / 32"""
    return _ro((np.asarray(rows, np.float64) / 32.0).astype(np.float16))


@functools.lru_cache(maxsize=None)
def identical_case():
    """300 copies of one row; queries: the row (1.0 everywhere: row 0 wins), its negation (-1.0 everywhere: row 0, -1.0), zeros"""
    rng = np.random.default_rng(300)
    g = exact_free_rows(rng, 1)
    return _ro(np.repeat(g, 300, axis=0), np.concatenate([g, -g, np.zeros((1, D), np.float32)]))


IDENTITY_N = 300


@functools.lru_cache(maxsize=None)
def identity_probe():
    """-> (G16 [300, 512] fp16 with G[r, k] = ((7 r + 13 k) mod 127 - 63) / 64, Q16 = the 512 one-hot rows e_k): S[k, r] == G[r, k]"""
    r, k = np.meshgrid(np.arange(IDENTITY_N), np.arange(D), indexing="ij")
    G = (((7 * r + 13 * k) % 127 - 63) / 64.0).astype(np.float16)
    return _ro(G, np.eye(D, dtype=np.float16))


def _odd_rows(rng, n):
    """rows with a few large and many tiny components, the tiny ones reaching down into the fp16 subnormals after normalisation"""
    x = 10.0 ** rng.uniform(-7.6, -3.5, size=(n, D)) * rng.choice([-1, 1], size=(n, D))
    for i in range(n):
        big = rng.permutation(D)[:4]
        x[i, big] = rng.uniform(0.3, 0.7, size=4) * rng.choice([-1, 1], size=4)
    return x


@functools.lru_cache(maxsize=None)
def general_case(N, M):
    """-> (G16 [N, 512], Q16 [M, 512]) fp16 unit rows.  Queries: a third planted at noise 0.3 / sqrt(512) per component, a third at
    0.05, near-ties between two rows, and (M >= 33) four odd rows; four odd rows in the gallery too (N >= 1000)"""
    rng = np.random.default_rng(7 * N + M)
    G = rng.standard_normal((N, D))
    n_odd = 4 if N >= 1000 else 0
    if n_odd:
        G[100:100 + n_odd] = _odd_rows(rng, n_odd)
    G = mm.normalize(G)
    Q = np.empty((M, D))
    planted = rng.integers(0, N, size=M)
    for m in range(M):
        kind = m % 3
        if kind == 0:
            Q[m] = G[planted[m]] + 0.3 / np.sqrt(D) * rng.standard_normal(D)
        elif kind == 1:
            Q[m] = G[planted[m]] + 0.05 * rng.standard_normal(D)
        else:                                                   # a near-tie: (almost) the same score on two rows
            other = int(rng.integers(0, N))
            Q[m] = G[planted[m]] + G[other] + 1e-4 * rng.standard_normal(D)
    if M >= 33:
        Q[5:9] = _odd_rows(rng, 4)
        Q[9] = G[100] if n_odd else Q[9]                        # an odd query on an odd row: tiny times tiny products
    return _ro(mm.to_f16(G), mm.to_f16(mm.normalize(Q)))


ORDINARY, ZERO, TOO_SMALL, TOO_LARGE, HAS_NAN, HAS_INF = range(6)


@functools.lru_cache(maxsize=None)
def normalization_rows():
    """-> (rows [n, 512] float32, kind [n]).  Gaussian rows scaled by 2^-30 ... 2^30, rows with one dominant entry, a zero row, one row
    below and one above the domain, a row with a NaN and one with +inf - each poisoned row among ordinary rows of its 4-row workgroup"""
    rng = np.random.default_rng(512)
    rows, kind = [], []
    for e in range(-30, 31, 3):
        rows.append(rng.standard_normal(D) * 2.0 ** e)
        kind.append(ORDINARY)
    for scale in (1e-3, 1e-6, 1.0):
        r = rng.standard_normal(D) * scale
        r[rng.integers(0, D)] = 40.0 * rng.choice([-1, 1])
        rows.append(r)
        kind.append(ORDINARY)
    while len(rows) % 4:
        rows.append(rng.standard_normal(D))
        kind.append(ORDINARY)
    for k in (ZERO, TOO_SMALL, TOO_LARGE, HAS_NAN, HAS_INF):     # one 4-row workgroup each: ordinary, ordinary, the odd one, ordinary
        group = [rng.standard_normal(D) * s for s in (1.0, 2.0 ** -9, 1.0, 2.0 ** 11)]
        if k == ZERO:
            group[2] = np.zeros(D)
        elif k == TOO_SMALL:
            group[2] = rng.standard_normal(D) * 2.0 ** -84      # every square below 2^-149
        elif k == TOO_LARGE:
            group[2] = rng.standard_normal(D) * 2.0 ** 70       # squares beyond 2^128 (2^40 < norm: outside the domain)
            group[2][np.abs(group[2]) < 2.0 ** 64.5] = 2.0 ** 66
        elif k == HAS_NAN:
            group[2][77] = np.nan
        else:
            group[2][400] = np.inf
        rows += group
        kind += [ORDINARY, ORDINARY, k, ORDINARY]
    with np.errstate(over="ignore"):
        return _ro(np.array(rows).astype(np.float32), np.array(kind))


# ---------------------------------------------------------------------------------------------------- inputs of the older matcher tests
def parity_inputs(N, M):
    """test_match_parity (tests/test_gpu_kernels.py)"""
    rng = np.random.default_rng(N * 7 + M)
    G = rng.standard_normal((N, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    planted = rng.integers(0, N, size=M)
    Q = G[planted] + 0.05 * rng.standard_normal((M, 512)).astype(np.float32) / np.sqrt(512) * 4
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    return G, Q


def topk_inputs(N, M, k):
    """test_match_topk_parity"""
    rng = np.random.default_rng(N + 31 * k)
    G = rng.standard_normal((N, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    if N >= 1000:
        G[700] = G[3]                       # exact duplicates: the lower row must come first
        G[701] = G[3]
    Q = G[rng.integers(0, N, size=M)] + 0.3 * rng.standard_normal((M, 512)).astype(np.float32) / np.sqrt(512)
    if N >= 1000:
        Q[0] = G[3]
    return G, Q


def running_best_inputs(N, M):
    """test_match_running_best_kernel_equals_per_tile_kernel"""
    rng = np.random.default_rng(N * 1000 + M)
    G = rng.standard_normal((N, 512)).astype(np.float32)
    if N > 64:
        G[N - 1] = G[7]                      # duplicates far apart: the lower row must win
        G[N // 2] = G[7]
    Q = rng.standard_normal((M, 512)).astype(np.float32)
    if N > 64:
        Q[0] = G[7]
    return G, Q


PARITY_SHAPES = [(1000, 5), (128, 1), (4097, 37), (10000, 320), (1, 3)]
TOPK_SHAPES = [(1000, 5, 7), (4097, 3, 64), (5, 2, 8), (100000, 4, 10)]
RUNNING_BEST_SHAPES = [(1, 1), (31, 5), (1000, 33), (4097, 320), (70001, 512), (300, 513)]
SNAPSHOT_ROWS_SEED = 23


def snapshot_rows():
    """test_every_way_to_install_a_gallery_snapshot_agrees: 40 non-unit fp32 rows"""
    rng = np.random.default_rng(SNAPSHOT_ROWS_SEED)
    return (rng.standard_normal((40, 512)) * rng.uniform(0.2, 3.0, (40, 1))).astype(np.float32)
