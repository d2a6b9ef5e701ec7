"""Float64 reference of the matcher (csrc/match.hip: match_kernel, match_top1_kernel, match_reduce_kernel, topk_rows_kernel,
within_sort_kernel) and of normalize_rows_kernel (csrc/aux_kernels.hip), with derived error bounds, plus fp32 transcriptions of the
kernels' arithmetic for the host tests.  Plain numpy; nothing here is read from the device or fitted to it.

normalize(x)        x / ||x|| in float64; a row whose sum of squares is 0 becomes a zero row, as the kernel defines (inv = 0).  A row
                    with a NaN is NaN throughout, a row with an infinity is zeros and a NaN there: every score of such a query is NaN.
to_f16(a)           the ONE rounding to the stored type, round to nearest even (numpy converts float64 -> float16 directly).
scores(g16, q16)    float64 product of the fp16 operands as given -> [M, N].  Exact zeros are +0 (what a chain of fp32 additions that
                    starts at +0 gives).
top1 / topk / within  selections under the total order (score descending, row ascending) on the score matrix handed in (the tests
                    hand in scores() rounded to float32: what the device selects on).  A NaN score is never selected or listed; a
                    query with nothing selectable gives -1 / -2.0.  Domain: scores in [-2, 2] or NaN - unit rows, or what
                    normalize_rows_kernel makes of a NaN / infinite row (zeros and one NaN: every score NaN).
score_bound(g16, q16)  512 * 2^-23 * (|q16| @ |g16|.T) per element.  Every product of two fp16 values is exact in fp32 (22
                    significand bits, exponent >= -48).  A sum of n such terms in ANY order - sequential, pairwise, the matrix unit's
                    internal tree - makes n - 1 additions; each rounds by at most one ulp of its result, relative 2^-23 whether it
                    rounds to nearest (2^-24) or truncates (2^-23), and each partial sum is bounded by the sum of the |terms| it
                    covers times (1 + 2^-23)^depth.  So |fl(sum) - sum| <= ((1 + 2^-23)^511 - 1) * sum|terms| < 512 * 2^-23 *
                    sum|terms|.  A derivation: never tightened from what the device shows.
normalize_bound(x)  per element: half an fp16 ulp at the exact value v = x / ||x|| (exponent floor 2^-14: subnormal spacing 2^-24)
                    + C_NORM * 2^-24 * |v|.  Within that distance of a rounding boundary either fp16 neighbour is accepted.  C_NORM
                    counts normalize_rows_kernel's fp32 roundings (unit roundoff u = 2^-24 each, all terms of ss are >= 0 so every
                    partial sum is <= ss):
                        ss:   1 (the product e*e) + 8 (the serial adds of a lane, the first one to 0 counted) + 6 (butterfly adds)
                              = 15 u on ss, HALVED by the square root                                                  7.5
                        sqrtf                                                                                          1
                        1.0f / .                                                                                       1
                        e[i] * inv                                                                                     1
                                                                                                                      10.5
                    and half a unit for every second-order term ((1 + u)^15 - 1 - 15 u < 2^-40) and for squares that fall below
                    the fp32 normal range (|x_i| < 2^-63 in a row of norm >= 2^-40: < 512 * 2^-149 / 2^-80 = 2^-60 of ss): C_NORM = 11.
                    DOMAIN: 2^-40 <= ||x|| <= 2^40.  Outside it the fp32 squares underflow (every |x_i| < 2^-75: ss = 0, inv = 0) or
                    overflow (ss = inf, inv = 1 / inf = 0) and the kernel returns a zero row; NaN and infinite rows give zeros and a NaN
                    where the NaN / infinity stood (0 * inf).
public_score_bound(g16, Q)  for queries Q (fp32 rows) that went through normalize_rows_kernel, against the reference scores on
                    q = to_f16(normalize(Q)): score_bound(g16, q) + normalize_bound(Q) @ |g16|.T.  The second term is the query-rounding
                    term: the device's fp16 query element is a neighbour of the exact value within normalize_bound of it, and equals
                    q's element unless the exact value sits within C_NORM * 2^-24 * |v| of a rounding boundary; a whole row's allowance
                    (512 half ulps) covers the few elements where the two roundings part.
fp32 emulations     scores_fp32 (sequential / pairwise / random order), normalize_fp32 (the kernel's order or a random one),
                    emulate_* with mutants: HOST TESTS ONLY (tests/test_match_inputs.py).  No GPU assertion compares against them.
"""
import numpy as np

D = 512
U23 = 2.0 ** -23
U24 = 2.0 ** -24
C_NORM_COUNT = {"ss (1 product + 8 serial adds + 6 butterfly adds) / 2": 7.5, "sqrtf": 1.0, "1.0f / x": 1.0, "e[i] * inv": 1.0,
                "second order, squares below the normal range": 0.5}
C_NORM = sum(C_NORM_COUNT.values())
NORM_MIN, NORM_MAX = 2.0 ** -40, 2.0 ** 40
NONE_IDX, NONE_COS = -1, np.float32(-2.0)


# ---------------------------------------------------------------------------------------------------- the reference
def normalize(x):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        n = np.sqrt((x * x).sum(-1, keepdims=True))
        return np.where(n == 0, 0.0, x / np.where(n == 0, 1.0, n))       # (a NaN row stays NaN; inf / inf is NaN, finite / inf is 0)


def to_f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16)


def scores(g16, q16):
    g = np.asarray(g16).astype(np.float64)
    q = np.asarray(q16).astype(np.float64)
    with np.errstate(all="ignore"):
        return q @ g.T + 0.0


def score_bound(g16, q16):
    g = np.abs(np.asarray(g16).astype(np.float64))
    q = np.abs(np.asarray(q16).astype(np.float64))
    return D * U23 * (q @ g.T)


def half_ulp_f16(v):
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


def normalize_bound(x):
    v = normalize(x)
    return half_ulp_f16(v) + C_NORM * U24 * np.abs(v)


def in_domain(x):
    n = np.sqrt((np.asarray(x, np.float64) ** 2).sum(-1))
    return (n >= NORM_MIN) & (n <= NORM_MAX)


def public_score_bound(g16, Q):
    """|S_dev - scores(g16, to_f16(normalize(Q)))| <= this, for queries Q (fp32 rows, in the domain) normalised by the device"""
    g = np.abs(np.asarray(g16).astype(np.float64))
    return score_bound(g16, to_f16(normalize(Q))) + normalize_bound(Q) @ g.T


def _first_k(srow, k):
    """rows of the first k entries of one score row under (score descending, row ascending), NaN left out"""
    valid = ~np.isnan(srow)
    nv = int(valid.sum())
    if nv == 0 or k <= 0:
        return np.zeros(0, np.int64)
    if nv <= k:
        cand = np.nonzero(valid)[0]
    else:
        vals = srow[valid]
        thr = np.partition(vals, nv - k)[nv - k]                     # the k-th largest
        with np.errstate(invalid="ignore"):
            cand = np.nonzero(valid & (srow >= thr))[0]
    return cand[np.argsort(-srow[cand], kind="stable")][:k]          # cand ascends: ties keep the lower row


def top1(S):
    """-> (idx [M] int32, cos [M] float32)"""
    S = np.asarray(S)
    nan = np.isnan(S)
    idx = np.where(nan, -np.inf, S).argmax(1)                        # the first of equal maxima: the lowest row
    none = nan.all(1)
    cos = S[np.arange(S.shape[0]), idx].astype(np.float32)
    return np.where(none, NONE_IDX, idx).astype(np.int32), np.where(none, NONE_COS, cos).astype(np.float32)


def topk(S, k):
    """-> (idx [M, k] int32, cos [M, k] float32), -1 / -2.0 behind the selectable rows"""
    S = np.asarray(S)
    M = S.shape[0]
    idx = np.full((M, k), NONE_IDX, np.int32)
    cos = np.full((M, k), NONE_COS, np.float32)
    for q in range(M):
        o = _first_k(S[q], k)
        idx[q, :len(o)] = o
        cos[q, :len(o)] = S[q, o]
    return idx, cos


def within(S, min_cos, cap):
    """-> (idx [M, cap] int32, cos [M, cap] float32, n_hits [M] int32): rows with score >= float32(min_cos); n_hits is the true count"""
    S = np.asarray(S)
    M = S.shape[0]
    idx = np.full((M, cap), NONE_IDX, np.int32)
    cos = np.full((M, cap), NONE_COS, np.float32)
    n = np.zeros(M, np.int32)
    with np.errstate(invalid="ignore"):
        hit = S >= np.float32(min_cos)
    for q in range(M):
        n[q] = hit[q].sum()
        if n[q]:
            o = _first_k(np.where(hit[q], S[q], np.nan), cap)
            idx[q, :len(o)] = o
            cos[q, :len(o)] = S[q, o]
    return idx, cos, n


# ---------------------------------------------------------------------------------------------------- the GPU file's predicates
def same_bits(got, want):
    """bit comparison of two arrays of the same shape and dtype (float32 as uint32, float16 as uint16: NaN payloads and -0 count)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    view = {np.dtype(np.float32): np.uint32, np.dtype(np.float16): np.uint16}.get(got.dtype)
    return bool(np.array_equal(got.view(view), want.view(view)) if view else np.array_equal(got, want))


def scores_within_bound(S_dev, g16, q16):
    """general family with the score matrix: |S_dev - scores()| <= score_bound, elementwise, no element left out"""
    return bool(np.all(np.abs(np.asarray(S_dev, np.float64) - scores(g16, q16)) <= score_bound(g16, q16)))


def worst_score(S_dev, g16, q16):
    """largest err / bound (reported, never asserted on its own)"""
    b = score_bound(g16, q16)
    return float((np.abs(np.asarray(S_dev, np.float64) - scores(g16, q16)) / np.maximum(b, 1e-300)).max())


def top1_within_bound(idx, cos, S_ref, B):
    """general family without a score matrix: with r the reference row of a query and b its bounds, the returned row i satisfies
    r[i] >= max(r) - 2 max(b) and |cos - r[i]| <= b[i]; every query is judged -> (ok, largest |cos - r[i]| / b[i])"""
    idx = np.asarray(idx, np.int64)
    M, N = S_ref.shape
    if idx.shape != (M,) or np.any(idx < 0) or np.any(idx >= N):
        return False, np.inf
    ar = np.arange(M)
    ri, bi = S_ref[ar, idx], B[ar, idx]
    err = np.abs(np.asarray(cos, np.float64) - ri)
    ok = np.all(ri >= S_ref.max(1) - 2.0 * B.max(1)) and np.all(err <= bi)
    return bool(ok), float((err / np.maximum(bi, 1e-300)).max())


def normalized_within_bound(got16, x):
    """|got - x / ||x||| <= normalize_bound on every element -> (ok, largest err / bound)"""
    err = np.abs(np.asarray(got16).astype(np.float64) - normalize(x))
    b = normalize_bound(x)
    with np.errstate(invalid="ignore"):
        ok = np.all(err <= b)                                        # (a NaN in got fails)
    return bool(ok), float((err / b).max())


# ---------------------------------------------------------------------------------------------------- fp32 emulations (host tests)
def _sum_f32(T, order, rng=None):
    """sum over the last axis of float32 terms T in fp32: 'seq', 'pair' (binary tree) or 'rand' (sequential over a permutation)"""
    T = np.asarray(T, np.float32)
    if order == "pair":
        while T.shape[-1] > 1:
            T = (T[..., 0::2] + T[..., 1::2]).astype(np.float32)
        return T[..., 0]
    ks = np.arange(T.shape[-1]) if order == "seq" else rng.permutation(T.shape[-1])
    acc = np.zeros(T.shape[:-1], np.float32)
    for k in ks:
        acc = (acc + T[..., k]).astype(np.float32)
    return acc


def scores_fp32(g16, q16, order="seq", rng=None, ksel=None):
    """[M, N] float32: the products (exact in fp32) summed in fp32 in the given order; ksel: the k positions that take part"""
    g = np.asarray(g16).astype(np.float32)
    q = np.asarray(q16).astype(np.float32)
    if ksel is not None:
        g, q = g[:, ksel], q[:, ksel]
    T = (q[:, None, :] * g[None, :, :]).astype(np.float32)
    return _sum_f32(T, order, rng)


def normalize_fp32(x, order="kernel", rng=None, truncate=False):
    """normalize_rows_kernel in numpy float32 -> float16 rows.  order 'kernel': lane l sums elements l, l + 64, ... serially, then the
    xor butterfly 32, 16, ... 1; 'seq' / 'rand': one serial sum.  truncate: the mutant that converts to fp16 towards zero."""
    f32 = np.float32
    x = np.asarray(x, f32)
    with np.errstate(all="ignore"):
        sq = (x * x).astype(f32)
        if order == "kernel":
            lanes = _sum_f32(sq.reshape(-1, 8, 64).transpose(0, 2, 1), "seq")        # [n, 64]
            for o in (32, 16, 8, 4, 2, 1):
                lanes = (lanes + lanes[:, np.arange(64) ^ o]).astype(f32)
            ss = lanes[:, 0]
        else:
            ss = _sum_f32(sq, order, rng)
        inv = np.where(ss > 0, f32(1.0) / np.sqrt(ss, dtype=f32), f32(0.0)).astype(f32)
        o = (x * inv[:, None]).astype(f32)
        if not truncate:
            return o.astype(np.float16)
        r = o.astype(np.float16)
        too_big = np.abs(r.astype(f32)) > np.abs(o)                                  # rounded away from zero: one step back
        return np.where(too_big, np.nextafter(r, np.float16(0)), r).astype(np.float16)


MUTANTS = ("drop_last_kstep", "swap_query_chunks", "swap_half_wave_rows", "ties_to_higher_row", "unmasked_tail", "strict_within",
           "truncating_f16", "minus_three_sentinel")


def emulate_scores(g16, q16, mutant=None):
    """the per-tile kernel's score matrix on a numpy emulation (sequential fp32 sum) [M, N]"""
    g = np.asarray(g16)
    q = np.asarray(q16)
    ksel = None
    if mutant == "drop_last_kstep":
        ksel = np.arange(D - 16)
    if mutant == "swap_query_chunks":                  # chunks 2 and 3 (8 halves each) of the query rows with (row & 15) == 5
        q = q.copy()
        rows = np.nonzero((np.arange(q.shape[0]) & 15) == 5)[0]
        a, b = q[rows, 16:24].copy(), q[rows, 24:32].copy()
        q[rows, 16:24], q[rows, 24:32] = b, a
    S = scores_fp32(g, q, "seq", ksel=ksel)
    if mutant == "swap_half_wave_rows":                # accumulator element <-> gallery row: the two half-waves exchanged (row ^ 4)
        N = g.shape[0]
        src = np.arange(N) ^ 4
        src = np.where(src < N, src, np.arange(N))
        S = S[:, src]
    return S


def emulate_top1(S, N_real=None, mutant=None):
    """top-1 of a score matrix as match_kernel + match_reduce_kernel select it.  N_real: S has columns beyond the gallery (the
    clamped copies of row N_real - 1 a block reads), which the kernel masks by g < N"""
    S = np.asarray(S, np.float32)
    if N_real is not None and mutant != "unmasked_tail":
        S = S[:, :N_real]
    M, N = S.shape
    idx = np.full(M, -1, np.int32)
    cos = np.full(M, -3.0 if mutant == "minus_three_sentinel" else -2.0, np.float32)
    for q in range(M):
        best, bi = np.float32(-3.0), -1
        for g in range(N):
            v = S[q, g]
            if v > best or (mutant == "ties_to_higher_row" and v == best and bi >= 0):
                best, bi = v, g
        if bi >= 0:
            idx[q], cos[q] = bi, best
    return idx, cos


def emulate_within(S, min_cos, cap, N_real=None, mutant=None):
    """hit lists as the within epilogue + within_sort_kernel + the rebuild of overflowed lists produce them"""
    S = np.asarray(S, np.float32)
    if N_real is not None and mutant != "unmasked_tail":
        S = S[:, :N_real]
    with np.errstate(invalid="ignore"):
        hit = S > np.float32(min_cos) if mutant == "strict_within" else S >= np.float32(min_cos)
    M = S.shape[0]
    idx = np.full((M, cap), -1, np.int32)
    cos = np.full((M, cap), -2.0, np.float32)
    n = hit.sum(1).astype(np.int32)
    for q in range(M):
        rows = np.nonzero(hit[q])[0]
        o = rows[np.argsort(-S[q, rows].astype(np.float64), kind="stable")][:cap]
        idx[q, :len(o)] = o
        cos[q, :len(o)] = S[q, o]
    return idx, cos, n
