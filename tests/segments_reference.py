"""numpy reference of the discretisation masks -> segment table (csrc/segments.hip), by brute force.

    activity   a[k, t] = sum_f masks[k, 0, t, f] / F                       (float64, and its float32 model)
    decision   b = a > threshold                                            (strict; NaN is inactive)
    closing    dilation (OR over the odd window, clipped to [0, T)), then erosion (AND, clipped): frames outside the row
               count as inactive for the one and as active for the other
    runs       maximal runs [s, e) of ones; e - s < min_frames dropped
    table      int32 rows (k, s, e) sorted by k, then s

Only numpy: the GPU tests import this file where scipy may be missing.  The windows are swept frame by frame on purpose
(the kernels work on runs and never sweep a window): the two share no code and no idea."""
import numpy as np


def check_params(dilation=1, erosion=1, min_frames=1):
    for name, w in (("dilation", dilation), ("erosion", erosion)):
        if int(w) != w or w < 1 or w % 2 == 0:
            raise ValueError(f"{name}={w!r}: an odd window >= 1")
    if int(min_frames) != min_frames or min_frames < 1:
        raise ValueError(f"min_frames={min_frames!r}: >= 1")


def activity64(masks):
    """masks [K, M, T, F] -> float64 [K, T], mask index 0"""
    m = np.asarray(masks)
    return m[:, 0].astype(np.float64).sum(-1) / m.shape[-1]


def activity32_exact(masks):
    """The float32 model where every partial sum is exact (masks multiples of 2^-10 in [0, 1], F <= 513): the exact sum,
    rounded to float32 (it is representable), then ONE float32 division by float32(F)."""
    m = np.asarray(masks)
    s = m[:, 0].astype(np.float64).sum(-1)
    s32 = s.astype(np.float32)
    assert (s32.astype(np.float64) == s).all(), "the sums are not exact in float32: the model does not apply"
    return s32 / np.float32(m.shape[-1])


def gamma(n):
    """Higham's gamma_n for float32: n u / (1 - n u), u = 2^-24"""
    u = 2.0 ** -24
    return n * u / (1 - n * u)


def decide(activity, threshold):
    a = np.asarray(activity)
    with np.errstate(invalid="ignore"):
        return a > a.dtype.type(threshold)


def _window(bits, w, op):
    bits = np.asarray(bits, dtype=bool)
    T = bits.shape[-1]
    h = w // 2
    out = np.empty_like(bits)
    for t in range(T):
        lo, hi = max(0, t - h), min(T, t + h + 1)                  # clipped
        out[..., t] = op(bits[..., lo:hi], axis=-1)
    return out


def dilate(bits, w):
    """d[t] = OR b[t - h .. t + h], h = w // 2, window clipped to [0, T)"""
    return _window(bits, w, np.any)


def erode(bits, w):
    """AND over the clipped window: what lies outside the row counts as active"""
    return _window(bits, w, np.all)


def closing(bits, dilation=1, erosion=1):
    return erode(dilate(bits, dilation), erosion)


def runs(row):
    """maximal runs [(s, e), ...] of ones in a 1-D bool row"""
    row = np.asarray(row, dtype=bool)
    out, s = [], None
    for t, v in enumerate(row):
        if v and s is None:
            s = t
        if not v and s is not None:
            out.append((s, t))
            s = None
    if s is not None:
        out.append((s, len(row)))
    return out


def table_from_bits(bits, min_frames=1):
    rows = [(k, s, e) for k, row in enumerate(np.asarray(bits, dtype=bool)) for s, e in runs(row) if e - s >= min_frames]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3)


def segments(activity, threshold=0.5, dilation=1, erosion=1, min_frames=1):
    """activity [K, T] (any float dtype; decided in that dtype) -> int32 [S, 3]: the bit route"""
    check_params(dilation, erosion, min_frames)
    return table_from_bits(closing(decide(activity, threshold), dilation, erosion), min_frames)


def segments_minmax(activity, threshold=0.5, dilation=1, erosion=1, min_frames=1):
    """The same through sliding max, sliding min, then the threshold (thresholding is monotone): padding -inf for the
    max and +inf for the min.  A NaN is made -inf first: inactive, as in the decision."""
    check_params(dilation, erosion, min_frames)
    a = np.array(activity, dtype=np.float64)
    a[np.isnan(a)] = -np.inf
    K, T = a.shape

    def slide(x, w, op, pad):
        h = min(w // 2, T)
        xp = np.concatenate([np.full((K, h), pad), x, np.full((K, h), pad)], axis=1)
        return np.stack([op(xp[:, t:t + 2 * h + 1], axis=1) for t in range(T)], axis=1)

    y = slide(slide(a, dilation, np.max, -np.inf), erosion, np.min, np.inf)
    return table_from_bits(y > np.float64(np.asarray(activity).dtype.type(threshold)), min_frames)


def intervals(table, K):
    out = [[] for _ in range(K)]
    for k, s, e in np.asarray(table).reshape(-1, 3):
        out[int(k)].append((int(s), int(e)))
    return out


def compare(count, table, want):
    """What the GPU tests assert: the count and the first `count` rows equal the reference table exactly, in order,
    int32.  Returns None or a message."""
    want = np.asarray(want).reshape(-1, 3)
    table = np.asarray(table)
    if table.dtype != np.int32 or table.ndim != 2 or table.shape[1] != 3:
        return f"table is {table.dtype} {table.shape}, int32 [S, 3] expected"
    if int(count) != len(want):
        return f"count {int(count)} != {len(want)}"
    got = table[:int(count)]
    if got.shape != want.shape or not np.array_equal(got, want):
        bad = np.flatnonzero((got != want).any(1)) if got.shape == want.shape else []
        i = int(bad[0]) if len(bad) else 0
        return f"row {i}: got {got[i].tolist() if len(got) > i else None}, want {want[i].tolist()} ({len(bad)} rows differ)"
    return None


def edge_rows(T, dilation, chunk=256, seed=0):
    """[R, T] float32 activities in {0, .25, .5, .75, 1, NaN} built to hit the edges at threshold 0.5: all zeros, all
    ones, runs touching frame 0 and frame T, single-frame spikes and gaps, gaps of dilation - 1, dilation and
    dilation + 1 frames, runs straddling every multiple of `chunk`, a NaN frame inside a run, frames exactly at the
    threshold, and random rows."""
    rs = np.random.RandomState(seed + 7919 * T + dilation)
    hi, lo = np.float32(1.0), np.float32(0.25)
    rows = [np.zeros(T, np.float32), np.ones(T, np.float32)]

    def blank():
        return np.full(T, lo, np.float32)

    r = blank(); r[:max(1, T // 5)] = hi; r[T - max(1, T // 7):] = hi; rows.append(r)           # touches 0 and T
    r = blank(); r[::3] = hi; rows.append(r)                                                     # spikes
    r = np.ones(T, np.float32); r[1::4] = lo; rows.append(r)                                     # single-frame gaps
    r = blank(); r[::2] = 0.75; rows.append(r)                                                   # ceil(T / 2) runs
    r = blank(); t = 1                                                                           # gaps around the window
    for g in (dilation - 1, dilation, dilation + 1, 1, 2, dilation + 1, dilation, dilation - 1):
        if t >= T:
            break
        r[t:t + 3] = hi
        t += 3 + max(g, 1)
    rows.append(r)
    r = blank()                                                                                  # chunk boundaries
    for c in range(chunk, T + chunk, chunk):
        r[max(0, c - 2):min(T, c + 2)] = hi
    rows.append(r)
    r = blank()
    for c in range(chunk, T, chunk):
        r[c - 1:c] = hi                                                                          # ends exactly at c
        if c + 1 < T:
            r[c + 1] = hi                                                                        # gap exactly at c
    rows.append(r)
    r = np.ones(T, np.float32); r[T // 2] = np.nan; rows.append(r)                               # a NaN frame
    r = blank(); r[: T // 2] = 0.5; r[T // 2:] = np.nextafter(np.float32(0.5), np.float32(1)); rows.append(r)   # == thr
    for p in (0.1, 0.5, 0.9):
        rows.append(np.where(rs.rand(T) < p, hi, lo).astype(np.float32))
    rows.append(rs.rand(T).astype(np.float32))
    return np.stack(rows)
