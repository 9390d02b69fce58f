"""What argmin / argmax must return, stated by brute force on numpy data, and the input families of the arg-reduction
tests (tests/test_argreduce_cpu.py, tests/test_gpu_argreduce.py). No GPU, no torch.argmax.

The rule (float32 and int32, op "max" or "min"):
  1. a NaN beats every number, for max and for min;
  2. otherwise the numerically largest (smallest) element wins, -0.0 == +0.0;
  3. among equal winners, and among several NaNs, the lowest position wins;
  4. the value is the input element at that position, bit for bit.
`first_extreme` maps every element to an ordered integer key (rules 1 and 2) and takes the first position of the
largest key (rule 3); values are compared by the callers as int32 bit patterns gathered at those positions (rule 4).
Three deliberately wrong rules stand beside it (WRONG_RULES): the tests assert that each of them disagrees with the
right one somewhere in the suite, so an implementation with that fault cannot pass."""
import numpy as np
import torch

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
WRONG_RULES = ("last_wins", "nans_skipped", "neg_zero_less")
NAN_BITS = (0x7FC00001, 0xFFC00123, 0x7F800055, 0xFFFFFFFF)  # quiet and signalling, both signs, different payloads


def as_numpy(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def keys(x, op: str, rule: str = "right") -> np.ndarray:
    """int64 keys: a larger key is a better element under `op`."""
    x = np.ascontiguousarray(as_numpy(x))
    assert x.dtype in (np.float32, np.int32) and op in ("max", "min")
    b = x.view(np.uint32).astype(np.int64)
    nan = np.zeros(x.shape, dtype=bool)
    if x.dtype == np.float32:
        a = b & 0x7FFFFFFF
        nan = a > 0x7F800000
        k = np.where(b >= 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)  # negative floats descend with their bits
        if rule != "neg_zero_less":
            k = np.where(a == 0, 0x80000000, k)
    else:
        k = b ^ 0x80000000
    if op == "min":
        k = 0xFFFFFFFF - k
    k = np.where(nan, 1 << 32, k)  # above every number, under both ops
    if rule == "nans_skipped":
        k = np.where(nan, -1, k)
    return k


def first_extreme(x, op: str, axis=None, rule: str = "right") -> np.ndarray:
    """int64 positions of the winner: in the flattened array (axis=None, a 0-d result) or along `axis`."""
    k = keys(x, op, rule)
    if axis is None:
        k, axis = k.reshape(-1), 0
    n = k.shape[axis]
    best = k == k.max(axis=axis, keepdims=True)
    if rule == "last_wins":
        return n - 1 - np.flip(best, axis=axis).argmax(axis=axis)
    return best.argmax(axis=axis)  # the first True


def identity_bits(dtype, op: str) -> int:
    if np.dtype(dtype) == np.float32:
        return 0xFF800000 if op == "max" else 0x7F800000
    return 0x80000000 if op == "max" else 0x7FFFFFFF


def segment_first_extreme(x, offsets, op: str, rule: str = "right"):
    """(value bits as int32 [S], flat int32 positions [S]): -1 and the identity for an empty segment. Offsets in order:
    the non-empty segments tile [offsets[0], offsets[S]) without gaps, so one reduceat per step takes them all."""
    x, o = np.ascontiguousarray(as_numpy(x)).reshape(-1), as_numpy(offsets).astype(np.int64)
    s = len(o) - 1
    idx = np.full(s, -1, dtype=np.int32)
    bits = np.full(s, identity_bits(x.dtype, op), dtype=np.uint32)
    full = o[1:] > o[:-1]
    if full.any():
        lo, hi = int(o[0]), int(o[-1])
        k, starts, lens = keys(x[lo:hi], op, rule), (o[:-1] - lo)[full], (o[1:] - o[:-1])[full]
        best = k == np.repeat(np.maximum.reduceat(k, starts), lens)
        pos = np.arange(lo, hi)
        if rule == "last_wins":
            idx[full] = np.maximum.reduceat(np.where(best, pos, -1), starts)
        else:
            idx[full] = np.minimum.reduceat(np.where(best, pos, hi), starts)
        bits[full] = x.view(np.uint32)[idx[full]]
    return bits.view(np.int32), idx


def bits_of(t) -> np.ndarray:
    a = as_numpy(t)
    return (a if a.ndim == 0 else np.ascontiguousarray(a)).view(np.int32)  # (ascontiguousarray makes a 0-d array 1-d)


def gathered_bits(x, pos, axis=None) -> np.ndarray:
    """The int32 bit patterns of x at positions `pos` (flat, or along axis)."""
    b = bits_of(x)
    if axis is None:
        return b.reshape(-1)[np.asarray(pos)]
    return np.take_along_axis(b, np.expand_dims(np.asarray(pos, dtype=np.int64), axis), axis).squeeze(axis)


# ---------------------------------------------------------------- families
def ties(shape, seed=0) -> np.ndarray:
    """round(randn * 4) / 4 clipped to [-2, 2], so that a row of 64 or more elements holds its extremum several times.
    Without the clip it does not: over 2000 rows the extremum is repeated in 25% of the rows of 64 elements and in 32%
    of the rows of 4096 (the tail of a normal thins faster than the quarter steps fill), short of the half that
    tests/test_argreduce_cpu.py asserts. With it the top step holds 3% of the elements: 67% of the rows of 64 and 91%
    of the rows of 128 repeat their extremum (the same 2000-row count)."""
    rng = np.random.default_rng(seed)
    return np.clip(np.round(rng.standard_normal(shape) * 4) / 4, -2, 2).astype(np.float32)


def i32(shape, seed=0) -> np.ndarray:
    """Full-range int32 with INT32_MIN and INT32_MAX planted (twice each where there is room)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(INT32_MIN, INT32_MAX, size=shape, dtype=np.int64, endpoint=True).astype(np.int32)
    f = x.reshape(-1)
    if f.size >= 2:
        at = rng.choice(f.size, size=min(4, f.size), replace=False)
        f[at[0::2]] = INT32_MIN
        f[at[1::2]] = INT32_MAX
    return x


def flat_equal(shape, dtype=np.float32, value=1.5) -> np.ndarray:
    return np.full(shape, value, dtype=dtype)


def floor(shape, dtype, op: str) -> np.ndarray:
    """The values that collide with an identity: all -inf / INT32_MIN for max, all +inf / INT32_MAX for min."""
    x = np.empty(shape, dtype=np.uint32)
    x[...] = identity_bits(dtype, op)
    return x.view(dtype)


def zeros(shape, seed=0) -> np.ndarray:
    """Mixed -0.0 / +0.0 only."""
    rng = np.random.default_rng(seed)
    return np.where(rng.integers(0, 2, size=shape) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)


def nans(shape, axis=None, seed=0) -> np.ndarray:
    """`ties` with two NaNs of different payload and sign planted per row (rows along `axis`; axis=None: the whole
    array is one row), plus every fifth row all NaN (payloads cycling)."""
    rng = np.random.default_rng(seed + 1)
    x = ties(shape, seed)
    rows = x.view(np.uint32).reshape(1, -1) if axis is None else np.moveaxis(x.view(np.uint32), axis, -1)
    n = rows.shape[-1]
    it = np.ndindex(*rows.shape[:-1])
    for r, at in enumerate(it):
        row = rows[at]
        if r % 5 == 4:
            row[...] = np.array([NAN_BITS[(r + k) % 4] for k in range(n)], dtype=np.uint32)
        elif n >= 2:
            p = rng.choice(n, size=2, replace=False)
            row[p[0]], row[p[1]] = NAN_BITS[r % 2], NAN_BITS[1 - r % 2]
    return x


def planted(shape, p: int, op: str, dtype=np.float32, axis=None) -> np.ndarray:
    """A constant background with the unique extremum at position p (flat, or along axis in every row)."""
    x = np.full(shape, 1, dtype=dtype)
    win = dtype(2) if op == "max" else dtype(0)
    if axis is None:
        x.reshape(-1)[p] = win
    else:
        np.moveaxis(x, axis, -1)[..., p] = win
    return x


def repeated_extremum_share(x, op: str, axis) -> float:
    """The share of rows (along axis) whose extremum occurs more than once."""
    k = keys(x, op)
    return float(((k == k.max(axis=axis, keepdims=True)).sum(axis=axis) > 1).mean())


def segment_offset_shapes(n: int):
    """Offsets over n elements with the edges the segment tests name: empty segments at the start, in the middle and at
    the end, offsets[0] > 0, offsets[S] < n, S = 1 and S > n."""
    a, b, c = n // 5, n // 2, (4 * n) // 5
    return {
        "empty_start_mid_end": [0, 0, 0, a, a, a, b, c, c, n, n, n],
        "inside": [min(3, n), a + 1, b, b, max(c, b), max(n - 2, c)],
        "one": [0, n],
        "one_inside": [min(1, n), max(n - 1, min(1, n))],
        "more_segments_than_elements": sorted(np.random.default_rng(n).integers(0, n + 1, size=n + 9).tolist()),
    }
