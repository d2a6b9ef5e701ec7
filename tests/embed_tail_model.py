"""Float64 reference of the embedder's tail - the split-K FC (csrc/conv_mfma.hip, the `p.ksplit > 1` branch) and l2norm_kernel
(csrc/aux_kernels.hip) - with a derived error bound, a transcription of conv_pick_ksplit (csrc/frp_internal.h) and an fp32 emulation
of both kernels with fault switches for the host tests.  Plain numpy; nothing here is read from the device or fitted to it.

reference(x, w, bias, n)   float64: v = x @ w.T + bias, v / ||v|| for the rows below n; a row with ss == 0 becomes zeros (inv = 0, as
                    the kernel defines it).  A row with a NaN or an infinity in x is NaN throughout (every weight of that k is non-zero
                    in the tests' inputs: v is +-inf or NaN everywhere, inf / inf is NaN).
pick_ksplit(...)    conv_pick_ksplit, line by line.
bound(x, w, bias, n, ks)   per element of emb and of emb16, for general operands.  Terms, each with the line it pays for:
    A.  v_dev against v.  Every product of two fp16 values is exact in fp32 (22 significand bits, exponent >= -48): the matrix unit adds
        exact terms (conv_mfma.hip: mfma_group).  A sum of K of them in ANY order - the unit's internal tree, the accumulator chain over
        the k-steps of a slice - makes K - 1 additions (match_model.score_bound's argument: each rounds by at most one ulp of its result,
        relative 2^-23 whether it rounds to nearest or truncates, and each partial sum is bounded by the sum of the |terms| it covers times
        (1 + 2^-23)^depth).  The l2norm kernel then makes ksplit + 1 more: `float a = bias[i]` and `a += partials[...]` once per slab
        (aux_kernels.hip: l2norm_kernel; one of them stands for the first addition of every slice being counted above already).  Without
        a split the conv epilogue adds the bias once (conv_common.h: conv_epilogue): K additions, covered by the same count with ks = 1.
            |v_dev - v| <= Bv = ((1 + 2^-23)^(K + ks) - 1) * (|x| @ |w|.T + |bias|)
    B.  the normalisation of v_dev against that of v, exactly (no first-order cut): with r = ||v||, beta = ||Bv|| < r,
            |v_dev_i / ||v_dev|| - v_i / r| <= Bv_i / (r - beta) + |v_i| * (2 sum_j |v_j| Bv_j + beta^2) / ((2 r - beta) * r * (r - beta))
        (the first term: the element's own error over the smaller norm; the second: | ||v_dev||^2 - r^2 | = |2 v.d + d.d|).
    C.  the kernel's own roundings (unit roundoff u = 2^-24, round to nearest: hipcc's default keeps sqrtf and the divide correctly
        rounded, the Makefile passes no fast-math flag), relative to |v_dev_i| / ||v_dev||:
            `ss += v[q] * v[q]`       the square: 1 rounding unfused; fused into the addition it is that addition's (never more)
                                      the thread's serial additions: ceil(D / 256) - 1 (the first one adds to 0.f: exact)
            wave_sum                  6 butterfly additions
            (w0 + w1) + (w2 + w3)     2 additions
                                      all terms >= 0, every partial sum <= ss: (1 + ceil(D / 256) - 1 + 6 + 2) u on ss, HALVED by the root
            sqrtf(ss)                 1
            1.0f / .                  1
            v[q] * inv                1
            second order              0.5 ((1 + u)^12 - 1 - 12 u < 2^-40; squares below the fp32 normal range: domain, below)
        C_TAIL(D) = (ceil(D / 256) + 8) / 2 + 3.5     (D = 512: 8.5)
        and 2^-149 for a result in the fp32 subnormal range.
    emb:    B + C_TAIL u (|v_i| / r + B) + 2^-149
    emb16:  that + half an fp16 ulp at (|exact| + that) - `(_Float16)o` rounds o, which lies within the emb bound of the exact value
            (match_model.normalize_bound's term, taken at the far end of the interval so that a binade boundary inside it is covered).
    DOMAIN: 2^-40 <= ||v|| <= 2^40 and beta < r / 2 (in_domain): the tests assert it for every finite row they hold to the bound.
exact_bits(v)       the exact family: v and ss are integers below 2^24 in any order and any split, so the device's vector IS v and the
                    result is fl(v * fl(1 / fl(sqrt(ss)))) in fp32 - numpy's float32 sqrt, divide and multiply round correctly - and its
                    one rounding to fp16.
emulate(...)        HOST TESTS ONLY (tests/test_embed_tail_inputs.py): both kernels in numpy float32 with an explicit slice order, the
                    slab workspace as a flat poisoned buffer, the kernel's wave_sum / (w0 + w1) + (w2 + w3) order for ss, and the
                    fault switches FAULTS.  No GPU assertion compares against it.
"""
import numpy as np

U23 = 2.0 ** -23
U24 = 2.0 ** -24
FLAG_OUT_F32 = 2
NORM_MIN, NORM_MAX = 2.0 ** -40, 2.0 ** 40
FILL32, FILL16 = np.uint32(0xFFFFFFFF), np.uint16(0xFFFF)
FAULTS = ("drop_slab", "dup_slab", "shift_slice", "skip_bias", "bias_per_slab", "stride_from_cap", "factor_from_cap")


# ---------------------------------------------------------------------------------------------------- conv_pick_ksplit
def pick_ksplit(M, Cout, Ktot, n_cu, flags=FLAG_OUT_F32, has_res=False):
    if not (flags & FLAG_OUT_F32) or has_res or (Ktot & 63) or M <= 0:
        return 1
    nk = Ktot // 64
    tiles = ((M + 255) // 256) * ((Cout + 127) // 128)
    if tiles * 4 > n_cu or nk < 64:
        return 1
    best = 1
    for s in range(2, nk // 8 + 1):
        if nk % s == 0 and tiles * s <= n_cu:
            best = s
    return best


def factor_steps(Cout, Ktot, n_cu, max_rows):
    """[(n, n + 1)] with n + 1 <= max_rows: the row counts either side of every step of pick_ksplit"""
    f = [pick_ksplit(n, Cout, Ktot, n_cu) for n in range(1, max_rows + 1)]
    return [(n, n + 1) for n in range(1, max_rows) if f[n - 1] != f[n]]


# ---------------------------------------------------------------------------------------------------- the reference
def f64(a):
    return np.asarray(a).astype(np.float64)


def pre_norm(x, w, bias, n):
    with np.errstate(all="ignore"):
        return f64(x)[:n] @ f64(w).T + f64(bias)


def normalize(v):
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        r = np.sqrt((v * v).sum(-1, keepdims=True))
        return np.where(r == 0, 0.0, v / np.where(r == 0, 1.0, r))


def reference(x, w, bias, n):
    return normalize(pre_norm(x, w, bias, n))


def to_f16(a):
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(np.float16)


def half_ulp_f16(v):
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 0.5 * 2.0 ** (e - 10)


def c_tail(D):
    return (-(-D // 256) + 8) / 2.0 + 3.5


def bound(x, w, bias, n, ks):
    """-> (ref [n, D], bound32 [n, D], bound16 [n, D], in_domain [n]); rows with a NaN / infinity carry NaN and False"""
    x, w, bias = f64(x)[:n], f64(w), f64(bias)
    K, D = x.shape[1], w.shape[0]
    with np.errstate(all="ignore"):
        v = x @ w.T + bias
        A = np.abs(x) @ np.abs(w).T + np.abs(bias)                      # A: the |terms| every addition's error is relative to
        Bv = ((1.0 + U23) ** (K + max(int(ks), 1)) - 1.0) * A           # A: K - 1 additions of products, ks + 1 in l2norm_kernel
        r = np.sqrt((v * v).sum(-1, keepdims=True))
        beta = np.sqrt((Bv * Bv).sum(-1, keepdims=True))
        ok = (r >= NORM_MIN) & (r <= NORM_MAX) & (beta < r / 2)
        zero = (r == 0) & (beta == 0)                                   # x row of zeros and zero bias: exact zeros, bound 0
        rs = np.where(ok, r, 1.0)
        B = Bv / (rs - beta) + np.abs(v) * (2.0 * (np.abs(v) * Bv).sum(-1, keepdims=True) + beta * beta) / ((2.0 * rs - beta) * rs * (rs - beta))   # B
        b32 = B + c_tail(D) * U24 * (np.abs(v) / rs + B) + 2.0 ** -149  # C
        ref = normalize(v)
        b32 = np.where(zero, 0.0, np.where(ok, b32, np.nan))
        b16 = b32 + np.where(zero, 0.0, half_ulp_f16(np.abs(ref) + b32))   # the rounding of `(_Float16)o`
    return ref, b32, b16, (ok | zero)[:, 0]


def within(got, ref, b):
    """every element inside its bound (a NaN in got or in the bound fails) -> (ok, largest err / bound)"""
    err = np.abs(f64(got) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = bool(np.all(err <= b))
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, np.inf))
    return ok, float(np.where(np.isnan(ratio), np.inf, ratio).max()) if ratio.size else 0.0


def exact_bits(v):
    """integer rows v (|v|, ss < 2^24) -> (emb float32, emb16 float16) as fp32 arithmetic gives them"""
    f32 = np.float32
    v64 = np.asarray(v, np.float64)
    ss = (v64 * v64).sum(-1)
    assert np.array_equal(v64, np.round(v64)) and ss.max(initial=0) < 2 ** 24
    with np.errstate(divide="ignore"):
        inv = np.where(ss > 0, f32(1.0) / np.sqrt(ss.astype(f32), dtype=f32), f32(0.0)).astype(f32)
    emb = (v64.astype(f32) * inv[:, None]).astype(f32)
    return emb, emb.astype(np.float16)


def same_bits(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    view = {np.dtype(np.float32): np.uint32, np.dtype(np.float16): np.uint16}[got.dtype]
    return bool(np.array_equal(got.view(view), want.view(view)))


def is_fill(a):
    """elementwise: still the 0xFF bytes the entry point put there"""
    a = np.asarray(a)
    return a.view(np.uint32) == FILL32 if a.dtype == np.float32 else a.view(np.uint16) == FILL16


# ---------------------------------------------------------------------------------------------------- fp32 emulation (host tests)
def _tree_f32(T):
    """pairwise fp32 sum over the last axis (an odd length is padded with a zero: adding 0 is exact)"""
    T = np.asarray(T, np.float32)
    while T.shape[-1] > 1:
        if T.shape[-1] & 1:
            T = np.concatenate([T, np.zeros(T.shape[:-1] + (1,), np.float32)], -1)
        T = (T[..., 0::2] + T[..., 1::2]).astype(np.float32)
    return T[..., 0]


def slice_sum(x, w, k0, k1, order):
    """[n, D] float32: sum over k in [k0, k1) of the (exact) products, k beyond K reads zeros (the buffer descriptor's range check).
    'seq': one fp32 accumulator over k; 'pair': a tree over 64-wide k-steps, then over the steps; 'blas': the exact sum rounded once"""
    K = x.shape[1]
    k1 = min(k1, K)
    xs, ws = x[:, k0:k1], w[:, k0:k1]
    with np.errstate(all="ignore"):
        if order == "blas":
            return (xs.astype(np.float64) @ ws.astype(np.float64).T).astype(np.float32)
        xf, wf = xs.astype(np.float32), ws.astype(np.float32)
        if order == "seq":
            acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
            for k in range(k1 - k0):
                acc = (acc + xf[:, k, None] * wf[None, :, k]).astype(np.float32)
            return acc
        steps = [_tree_f32(xf[:, None, k:k + 64] * wf[None, :, k:k + 64]) for k in range(0, k1 - k0, 64)]
        return _tree_f32(np.stack(steps, -1))


def conv_slabs(x, w, n, ks, order="blas", shift_slice=None):
    """the split-K conv: [ks, n, D] raw fp32 partial sums, slice s over k-steps [s * nk, (s + 1) * nk).  shift_slice: that slice's range
    starts and ends one 64-wide k-step late"""
    K = x.shape[1]
    per = K // ks
    assert per * ks == K and per % 64 == 0
    out = np.empty((ks, n, w.shape[0]), np.float32)
    for s in range(ks):
        off = 64 if s == shift_slice else 0
        out[s] = slice_sum(x[:n], w, s * per + off, (s + 1) * per + off, order)
    return out


def l2norm_rows(v):
    """l2norm_kernel behind the reduction: v [n, D] float32 -> (emb float32, emb16 float16).  Thread t holds elements t, t + 256, ...;
    ss: the thread's serial sum, the xor butterfly 32 .. 1 inside each of the 4 waves, (w0 + w1) + (w2 + w3)"""
    f32 = np.float32
    n, D = v.shape
    with np.errstate(all="ignore"):
        pad = np.zeros((n, 1024), f32)
        pad[:, :D] = (v * v).astype(f32)
        lanes = np.zeros((n, 256), f32)
        for q in range(4):
            lanes = (lanes + pad[:, q * 256:(q + 1) * 256]).astype(f32)
        lanes = lanes.reshape(n, 4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            lanes = (lanes + lanes[:, :, np.arange(64) ^ o]).astype(f32)
        ws = lanes[:, :, 0]
        ss = ((ws[:, 0] + ws[:, 1]).astype(f32) + (ws[:, 2] + ws[:, 3]).astype(f32)).astype(f32)
        inv = np.where(ss > 0, f32(1.0) / np.sqrt(ss, dtype=f32), f32(0.0)).astype(f32)
        emb = (v * inv[:, None]).astype(f32)
        return emb, emb.astype(np.float16)


def emulate(x, w, bias, n, cap, ks, order="blas", fault=None, fault_slab=0, ks_cap=None, slabs=None):
    """both kernels -> (emb [cap, D] float32, emb16 [cap, D] float16), rows at or beyond n holding the 0xFF fill.
    ks: the factor both kernels use (1: no split - the conv's fp32 epilogue adds the bias, plain l2norm); ks_cap: the factor of `cap` rows
    (factor_from_cap).  slabs: conv_slabs(...) of the same case, to spare the host tests the recomputation.
    The workspace is a flat fp32 buffer of NaNs (the 0xFF fill) that the conv writes with stride n; a read beyond it is a NaN too."""
    f32 = np.float32
    D = w.shape[0]
    bias = np.asarray(bias, f32)
    emb = np.full((cap, D), FILL32, np.uint32).view(f32)
    emb16 = np.full((cap, D), FILL16, np.uint16).view(np.float16)
    if n == 0:
        return emb, emb16
    with np.errstate(all="ignore"):
        if ks <= 1:
            acc = slice_sum(x[:n], w, 0, x.shape[1], order)
            v = acc if fault == "skip_bias" else (acc + bias).astype(f32)
        else:
            if fault == "shift_slice":
                slabs = np.array(slabs if slabs is not None else conv_slabs(x, w, n, ks, order))
                per = x.shape[1] // ks
                slabs[fault_slab] = slice_sum(x[:n], w, fault_slab * per + 64, (fault_slab + 1) * per + 64, order)
            elif slabs is None:
                slabs = conv_slabs(x, w, n, ks, order)
            ks_l2 = ks_cap if fault == "factor_from_cap" else ks
            M = cap if fault == "stride_from_cap" else n
            ws = np.full(max(ks, ks_l2) * cap * D + D, np.nan, f32)
            ws[:ks * n * D] = slabs.reshape(-1)                                       # [ks][n][D]: the conv's stride is the count n
            a = np.zeros((n, D), f32) if fault == "skip_bias" else np.tile(bias, (n, 1))
            rows = np.arange(n)[:, None]
            for s in range(ks_l2):
                if fault == "drop_slab" and s == fault_slab:
                    continue
                idx = np.minimum((s * M + rows) * D + np.arange(D)[None, :], ws.size - 1)
                for _ in range(2 if fault == "dup_slab" and s == fault_slab else 1):
                    a = (a + ws[idx]).astype(f32)
                if fault == "bias_per_slab" and s > 0:
                    a = (a + bias).astype(f32)
            v = a
        emb[:n], emb16[:n] = l2norm_rows(v)
    return emb, emb16
