"""CPU model, operand families and assertion functions for the device-wide reduce, dot and scan tests (torch and numpy
only, no GPU).

test_gpu_reduce_scan.py calls the assertion functions below on the kernels' results; test_reduce_oracle_cpu.py calls
the same functions on `emulate` (a float32 / int32 walk in the order csrc/kernels/reduce.hip uses) and on single-fault
mutants of it, which is the proof that they discriminate.

The model of reduce.hip (kThreads 256, kUnroll 4, kMaxBlocks 16384, kV 16)
  pass 1  n4 = n >> 2 float4 vectors; nb = clamp(ceil(n4 / 1024), 1, max_blocks) blocks; step = nb * 1024. Thread t of
          block b starts at vector i = 1024 b + t. UNROLLED loop: while i + 768 < n4, slot u in 0..3 takes vector
          i + 256 u, then i += step (one grid-stride TRIP). CLEAN-UP loop: while i < n4, slot 0 takes vector i, then
          i += 256 (at most three turns, all inside the block's own 1024-vector chunk of that trip). TAIL: thread
          t < (n & 3) of block 0 takes element 4 n4 + t into slot 1. A sum folds a vector as (x + y) + (z + w); min and
          max fold x, y, z, w one after the other into the slot, so a NaN is always the right-hand operand of
          `b < a ? b : a` and is skipped. Slots are merged 0 <- 1, 2, 3, lanes by a 6-step xor butterfly, the four
          waves in order by thread 0.
  pass 2  one block; the np = nb partials are read as np >> 2 float4s, thread t taking vectors t, t + 256, ... (16 per
          thread, out-of-range ones filled with the identity), component c into wide accumulator c (f64 / i64); thread
          t < (np & 3) adds partial 4 (np >> 2) + t to accumulator 0; (a0 + a1) + (a2 + a3), butterfly, waves in order.

depth(n, max_blocks, prod): the largest number of float32 roundings an input element goes through before the f64 fold
  2 (in-vector tree) + the most takes any one slot sees (the accumulator chain: one addition per trip, clean-up turn or
  tail element) + 3 (slot merge) + 6 (wave butterfly) + 3 (LDS fold of the four waves) [+ 1 for the product of a dot].
  Each rounding is at most 2^-24 relative to a partial sum that is at most sum|x| (1 + 2^-24)^depth, so
  |float32 partial sums - exact| <= depth 2^-24 sum|x| (1 + O(depth 2^-24)); pass 2 is f64 and its one rounding back to
  float32 adds 2^-24 |result|. The (1 + 2^-10) factor of `sum_bound` covers the second-order terms and the f64 fold.

scan_depth(i, n): the same count for output i of the production scan (scan.hip, 16 rows x 8 waves, 32768 per tile).
  With i = 32768 tile + 4096 wave + 256 row + 4 lane + comp, an element of the same tile goes through at most
  3 (in-row x, y, z, w chain) + 6 (wave scan of the lane totals) + (row, or 16 when it lies in an earlier wave: the
  carry chain over the rows) + 1 (carry + excl) + wave (the wave totals, added in order) + 1 (wexcl + lane_excl)
  + 1 (prefix + value) + 1 (the tile's offset) additions. An element of an earlier tile goes through 3 + 6 + 16 + 8
  (its tile's aggregate: rows, then the 8 wave totals) and then the look-back: at worst every predecessor is found
  inclusive at once, so the value hops tile by tile, each hop one accumulator addition, a 6-step butterfly and the
  `prefix + aggregate` of the republication: 8 per hop, `tile` hops; then init + prefix and the offset addition.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
THREADS, UNROLL, CAP, PASS2_VECS, WAVE = 256, 4, 16384, 16, 64  # reduce.hip: kThreads, kUnroll, kMaxBlocks, kV
CHUNK = THREADS * UNROLL  # float4 vectors one block takes per trip
TILE, SCAN_ROWS, SCAN_WAVES = 32768, 16, 8  # scan.hip: kTileElems and the production tile shape
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
OPS = ("sum", "min", "max")
UNROLLED, CLEANUP = 0, 1

FAULTS = (
    "tail_every_block",      # 1  the n & 3 tail is read by every block
    "tail_dropped",          # 2
    "dot_tail_xx",           # 3  the tail of the dot multiplies x[t] * x[t]
    "cleanup_short",         # 4  the clean-up loop stops one stride early
    "no_second_trip",        # 5  the grid-stride loop runs once
    "stride_off",            # 6  the stride is one block too long
    "slot3_reads_slot2",     # 7
    "pass2_tail_dropped",    # 8
    "pass2_fill_zero",       # 9  out-of-range pass-2 vectors are 0, not the identity
    "dot_y_from_x",          # 10 the vector loops read y4 from x4
    "sum_identity_negzero",  # 11
    "min_hands_on_nan",      # 12
    "minmax_tree",           # 13 min / max fold a vector as a tree: a NaN in x hides y, z, w; one in z hides w
)


def pass1_blocks(n: int, max_blocks: int = CAP) -> int:
    return int(min(max(((n >> 2) + CHUNK - 1) // CHUNK, 1), max_blocks))


# ------------------------------------------------------------------------------------------ the model: who takes what
@functools.lru_cache(maxsize=32)
def _rounds(n: int, max_blocks: int, fault: str | None, block_range: tuple[int, int] | None = None):
    """Pass 1 as index arithmetic: a list of rounds (region, slot, threads, vectors, trips), in program order for
    every thread (its unrolled trips, then its clean-up turns), and the tail as (threads, elements). A thread appears
    at most once per round. block_range: only the threads of blocks [b0, b1) (the tail belongs to block 0)."""
    n4, nb = n >> 2, pass1_blocks(n, max_blocks)
    step = (nb + 1 if fault == "stride_off" else nb) * CHUNK
    b0, b1 = (0, nb) if block_range is None else block_range
    tid = np.arange(b0 * THREADS, min(b1, nb) * THREADS, dtype=np.int64)
    i = (tid // THREADS) * CHUNK + tid % THREADS
    trips_done = np.zeros_like(tid)
    alive = np.ones(tid.shape, bool)
    rounds = []
    while True:
        alive = alive & (i + (UNROLL - 1) * THREADS < n4)
        if not alive.any():
            break
        for u in range(UNROLL):
            src = 2 if (u == 3 and fault == "slot3_reads_slot2") else u
            rounds.append((UNROLLED, u, tid[alive], i[alive] + src * THREADS, trips_done[alive].copy()))
        i[alive] += step
        trips_done[alive] += 1
        if fault == "no_second_trip":
            i[alive] = n4
            break
    while True:
        m = (i + THREADS < n4) if fault == "cleanup_short" else (i < n4)
        if not m.any():
            break
        rounds.append((CLEANUP, 0, tid[m], i[m].copy(), trips_done[m].copy()))
        i[m] += THREADS
    r = n & 3
    if fault == "tail_dropped":
        tail_threads = np.zeros(0, np.int64)
    elif fault == "tail_every_block":
        tail_threads = (np.arange(nb)[:, None] * THREADS + np.arange(r)[None, :]).reshape(-1)
    else:
        tail_threads = np.arange(r, dtype=np.int64)
    if b0 > 0:
        tail_threads = tail_threads[:0]
    tail_elems = (n4 << 2) + tail_threads % THREADS
    return rounds, (tail_threads, tail_elems), nb, step


def coverage(n: int, max_blocks: int = CAP, prod: bool = False, fault: str | None = None) -> SimpleNamespace:
    """Which block, thread and slot takes every input element, through which loop and on which trip, and how often;
    which pass-2 thread and component takes every partial. A correct model has vec_count, tail_count and part_count
    all ones (`exactly_once`)."""
    rounds, (tail_threads, tail_elems), nb, step = _rounds(n, max_blocks, fault)
    n4, r = n >> 2, n & 3
    c = SimpleNamespace(n=n, n4=n4, nb=nb, step=step, max_blocks=max_blocks, prod=prod)
    c.vec_count = np.zeros(n4, np.int64)
    for name in ("vec_thread", "vec_slot", "vec_region", "vec_trip"):
        setattr(c, name, np.full(n4, -1, np.int64))
    takes = np.zeros((nb * THREADS, UNROLL), np.int64)  # additions into every accumulator slot
    c.regions = {}
    for region, slot, threads, vecs, trips in rounds:
        c.vec_count += np.bincount(vecs, minlength=n4)
        c.vec_thread[vecs], c.vec_slot[vecs], c.vec_region[vecs], c.vec_trip[vecs] = threads, slot, region, trips
        takes[threads, slot] += 1
        for t in np.unique(trips):
            key = ("unrolled" if region == UNROLLED else "cleanup", int(t))
            c.regions[key] = c.regions.get(key, 0) + int((trips == t).sum())
    c.vec_block = np.where(c.vec_thread >= 0, c.vec_thread // THREADS, -1)
    c.tail_count = np.bincount(tail_elems - (n4 << 2), minlength=r) if r else np.zeros(0, np.int64)
    c.tail_threads = tail_threads
    np.add.at(takes, (tail_threads, 1), 1)
    if r:
        c.regions[("tail", 0)] = r
    c.elem_count = np.concatenate([np.repeat(c.vec_count, 4), c.tail_count])
    c.trips = 1 + max([int(t.max()) for *_, t in rounds], default=0)
    c.cleanup_taken = any(reg == CLEANUP for reg, *_ in rounds)
    c.tail_taken = r > 0
    # pass 2
    p4, c.np_tail = nb >> 2, nb & 3
    c.part_count = np.zeros(nb, np.int64)
    c.part_thread, c.part_comp = np.full(nb, -1, np.int64), np.full(nb, -1, np.int64)
    c.fill_live = 0
    if p4 > 0:
        for u in range(PASS2_VECS):
            v = u * THREADS + np.arange(THREADS)
            ok = v < p4
            c.fill_live += int((~ok).sum())
            for comp in range(4):
                idx = 4 * v[ok] + comp
                c.part_count[idx] += 1
                c.part_thread[idx], c.part_comp[idx] = np.arange(THREADS)[ok], comp
    if fault != "pass2_tail_dropped":
        idx = 4 * p4 + np.arange(c.np_tail)
        c.part_count[idx] += 1
        c.part_thread[idx], c.part_comp[idx] = np.arange(c.np_tail), 0
    c.depth = 2 + int(takes.max()) + 3 + 6 + 3 + (1 if prod else 0)
    c.exactly_once = bool((c.elem_count == 1).all() and (c.part_count == 1).all())
    return c


def coverage_counts(n: int, max_blocks: int = CAP, batch: int = 1024) -> SimpleNamespace:
    """The counts of `coverage` alone, walked in batches of blocks: for sizes whose per-vector tables would be large
    (2^26 elements and more). vec_count is uint8."""
    n4, nb = n >> 2, pass1_blocks(n, max_blocks)
    c = SimpleNamespace(n=n, n4=n4, nb=nb, vec_count=np.zeros(n4, np.uint8), tail_count=np.zeros(n & 3, np.int64),
                        trips=0, regions={}, max_takes=0)
    for b0 in range(0, nb, batch):
        rounds, (tail_threads, tail_elems), _, _ = _rounds.__wrapped__(n, max_blocks, None, (b0, b0 + batch))  # not cached
        takes = np.zeros((batch * THREADS, UNROLL), np.int32)
        for region, slot, threads, vecs, trips in rounds:
            lo, hi = int(vecs.min()), int(vecs.max()) + 1
            c.vec_count[lo:hi] += np.bincount(vecs - lo, minlength=hi - lo).astype(np.uint8)
            takes[threads - b0 * THREADS, slot] += 1
            c.trips = max(c.trips, 1 + int(trips.max()))
            for t in np.unique(trips):
                key = ("unrolled" if region == UNROLLED else "cleanup", int(t))
                c.regions[key] = c.regions.get(key, 0) + int((trips == t).sum())
        np.add.at(c.tail_count, tail_elems - (n4 << 2), 1)
        np.add.at(takes, (tail_threads, 1), 1)
        c.max_takes = max(c.max_takes, int(takes.max()))
    c.depth = 2 + c.max_takes + 3 + 6 + 3
    c.exactly_once = bool((c.vec_count == 1).all() and (c.tail_count == 1).all())
    return c


def depth(n: int, max_blocks: int = CAP, prod: bool = False) -> int:
    return coverage(n, max_blocks, prod).depth


def block_of_element(n: int, max_blocks: int = CAP) -> np.ndarray:
    c = coverage(n, max_blocks)
    return np.concatenate([np.repeat(c.vec_block, 4), np.zeros(n & 3, np.int64)])


# ------------------------------------------------------------------------------------------ the model: the arithmetic
def _identity(op, dtype, fault=None):
    if op == "sum":
        return dtype.type(-0.0) if (fault == "sum_identity_negzero" and dtype.kind == "f") else dtype.type(0)
    if dtype.kind == "f":
        return dtype.type(np.inf if op == "min" else -np.inf)
    return dtype.type(I32_MAX if op == "min" else I32_MIN)


def _comb(op, a, b, fault=None):
    """comb(a, b) of reduce.hip: a + b, b < a ? b : a, b > a ? b : a (a NaN in b is skipped, one in a stays)."""
    if op == "sum":
        return a + b
    if op == "min":
        if fault == "min_hands_on_nan":
            return np.where((b < a) | np.isnan(b), b, a)
        return np.where(b < a, b, a)
    return np.where(b > a, b, a)


def _block_fold(op, v, fault):
    """Wave butterfly (xor 32 .. 1) then the waves in order: v has one row per block, one column per thread."""
    w = v.reshape(v.shape[0], -1, WAVE)
    lane = np.arange(WAVE)
    off = WAVE // 2
    while off:
        w = _comb(op, w, w[:, :, lane ^ off], fault)
        off >>= 1
    r = w[:, 0, 0]
    for k in range(1, w.shape[1]):
        r = _comb(op, r, w[:, k, 0], fault)
    return r


def emulate(op: str, x: torch.Tensor, y: torch.Tensor | None = None, max_blocks: int | None = None,
            fault: str | None = None):
    """The result of reduce.hip's two passes on x (float32 or int32; y: the dot's second operand), computed on the CPU
    in the kernels' order and number formats. Returns a numpy scalar of x's type."""
    max_blocks = CAP if max_blocks is None else max_blocks
    xs = x.detach().reshape(-1).numpy()
    n, dt = xs.size, xs.dtype
    ys = None if y is None else y.detach().reshape(-1).numpy()
    rounds, (tail_threads, tail_elems), nb, _ = _rounds(n, max_blocks, fault)
    n4 = n >> 2
    x4 = xs[:n4 * 4].reshape(n4, 4)
    y4 = None if ys is None else (x4 if fault == "dot_y_from_x" else ys[:n4 * 4].reshape(n4, 4))
    with np.errstate(all="ignore"):
        acc = np.full((nb * THREADS, UNROLL), _identity(op, dt, fault), dt)
        for _, slot, threads, vecs, _ in rounds:
            v = x4[vecs]
            if y4 is not None:
                v = v * y4[vecs]
            a = acc[threads, slot]
            if op == "sum":
                a = a + ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3]))
            elif fault == "minmax_tree":
                a = _comb(op, a, _comb(op, _comb(op, v[:, 0], v[:, 1], fault), _comb(op, v[:, 2], v[:, 3], fault), fault), fault)
            else:
                for comp in range(4):
                    a = _comb(op, a, v[:, comp], fault)
            acc[threads, slot] = a
        if tail_threads.size:
            v = xs[tail_elems]
            if ys is not None:
                v = v * (xs[tail_elems] if fault == "dot_tail_xx" else ys[tail_elems])
            acc[tail_threads, 1] = _comb(op, acc[tail_threads, 1], v, fault)
        a = acc[:, 0]
        for u in range(1, UNROLL):
            a = _comb(op, a, acc[:, u], fault)
        partials = _block_fold(op, a.reshape(nb, THREADS), fault)
        # pass 2
        wt = np.dtype(np.float64 if dt.kind == "f" else np.int64)
        wid = _identity(op, wt, fault)
        acc2 = np.full((THREADS, 4), wid, wt)
        p4 = nb >> 2
        if p4 > 0:
            fill = dt.type(0) if fault == "pass2_fill_zero" else _identity(op, dt)
            pv = partials[:p4 * 4].reshape(p4, 4)
            for u in range(PASS2_VECS):
                i = u * THREADS + np.arange(THREADS)
                v = np.where((i < p4)[:, None], pv[np.minimum(i, p4 - 1)], fill).astype(wt)
                acc2 = _comb(op, acc2, v, fault)
        k = 0 if fault == "pass2_tail_dropped" else nb & 3
        if k:
            acc2[:k, 0] = _comb(op, acc2[:k, 0], partials[p4 * 4:p4 * 4 + k].astype(wt), fault)
        a = _comb(op, _comb(op, acc2[:, 0], acc2[:, 1], fault), _comb(op, acc2[:, 2], acc2[:, 3], fault), fault)
        r = _block_fold(op, a.reshape(1, THREADS), fault)[0]
        return r.astype(dt) if dt.kind == "f" else np.int64(r).astype(dt)


def model_run(fault: str | None = None):
    """The runner the assertion functions take, on the CPU model: run(op, x, y, max_blocks) -> numpy scalar."""
    def run(op, x, y=None, max_blocks=None):
        return emulate("sum" if op == "dot" else op, x, y, max_blocks, fault)
    return run


# ------------------------------------------------------------------------------------------ scan: depth and emulation
def scan_depth(i, n: int):
    """Roundings behind output i of an n-element production scan (module docstring); i may be an array."""
    i = np.asarray(i, dtype=np.int64)
    tile, e = i // TILE, i % TILE
    wave, row = e // (SCAN_ROWS * 256), (e % (SCAN_ROWS * 256)) // 256
    local = 3 + 6 + np.where(wave > 0, SCAN_ROWS, row) + 1 + wave + 1 + 1 + 1
    carried = 3 + 6 + SCAN_ROWS + SCAN_WAVES + 8 * tile + 2
    return np.where(tile > 0, np.maximum(local, carried), local)


def emulate_scan(x: torch.Tensor, exclusive: bool = False, init: float = 0.0) -> np.ndarray:
    """The production scan in float32 in the kernel's order, every look-back finding its predecessor inclusive (the
    longest chain of roundings the look-back can produce)."""
    xs = x.detach().reshape(-1).numpy().astype(np.float32)
    n = xs.size
    out = np.empty(n, np.float32)
    prefix = np.float32(0)
    f = np.float32
    for t in range((n + TILE - 1) // TILE):
        v = np.zeros(TILE, f)
        m = min(TILE, n - t * TILE)
        v[:m] = xs[t * TILE:t * TILE + m]
        v = v.reshape(SCAN_WAVES, SCAN_ROWS, WAVE, 4).copy()
        for c in range(1, 4):
            v[..., c] += v[..., c - 1]
        incl = v[..., 3].copy()  # [wave, row, lane]
        off = 1
        while off < WAVE:
            sh = np.zeros_like(incl)
            sh[..., off:] = incl[..., :-off]
            incl = incl + sh  # lanes below off add an exact zero
            off <<= 1
        excl = np.concatenate([np.zeros_like(incl[..., :1]), incl[..., :-1]], -1)
        carry = np.zeros((SCAN_WAVES,), f)
        lane_excl = np.empty_like(incl)
        for r in range(SCAN_ROWS):
            lane_excl[:, r] = carry[:, None] + excl[:, r]
            carry = carry + incl[:, r, -1]
        wexcl, agg = np.zeros(SCAN_WAVES, f), f(0)
        for w in range(SCAN_WAVES):
            wexcl[w + 1:] = wexcl[w + 1:] + carry[w]
            agg = f(agg + carry[w])
        b = wexcl[:, None, None] + lane_excl
        if exclusive:
            o = np.stack([b, b + v[..., 0], b + v[..., 1], b + v[..., 2]], -1)
        else:
            o = v + b[..., None]
        o = (o + f(f(init) + prefix)).reshape(-1)
        out[t * TILE:t * TILE + m] = o[:m]
        prefix = f(prefix + agg)
    return out


# ------------------------------------------------------------------------------------------ operand families
def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=8)
def _exact_pool(seed: int, dtype):
    n = 1 << 19
    g = _gen(seed)
    half = torch.randint(-8, 9, (n // 2,), generator=g)
    x = torch.stack([half, -half.roll(1)], 1).reshape(-1)  # balanced: the values cancel in pairs one step apart
    return x.to(dtype)


def exact_family(n: int, seed: int = 1, dtype=torch.float32):
    """Integers in [-8, 8] with balanced signs: (x, int64 sum). `assert_order_free` checks that no summation order can
    round."""
    pool = _exact_pool(seed, dtype)
    x = pool[:n].clone() if n <= pool.numel() else pool.repeat((n + pool.numel() - 1) // pool.numel())[:n].clone()
    return x, int(x.long().sum())


def weighted_family(n: int, seed: int = 0, dtype=torch.float32):
    """x[i] = +-(1 + (i + seed) mod 251), signs alternating: a dropped and a doubled element cannot cancel, a shifted
    read changes the sum. (x, int64 sum)."""
    i = torch.arange(n, dtype=torch.int64)
    x = (1 + (i + seed) % 251) * (1 - 2 * (i & 1))
    return x.to(dtype), int(x.sum())


def dot_partner(n: int, seed: int = 5):
    """The second operand of an exact dot: random integers in [-3, 3] (with the weighted family's 251 the products
    of one block's share still sum below 2^24 in magnitude; `assert_order_free` checks it)."""
    g = _gen(seed)
    return torch.randint(-3, 4, (n,), generator=g).float()


def assert_order_free(x: torch.Tensor, n: int, max_blocks: int, y: torch.Tensor | None = None):
    """Every float32 partial sum the kernel can form is exact: the largest sum |x| inside one block's share (any sum
    pass 1 forms is a sub-sum of one block's elements) and the total stay below 2^24. Pass 2 is f64."""
    v = x.double() if y is None else x.double() * y.double()
    per_block = np.bincount(block_of_element(n, max_blocks), weights=v.abs().numpy(), minlength=1) if n else np.zeros(1)
    assert per_block.max() < 2 ** 24 and abs(float(v.sum())) < 2 ** 24, (n, max_blocks, per_block.max())


def dense_family(n: int, seed: int = 2):
    """Signed float32 with all 24 mantissa bits in use over five binades: (x, float64 sum, float64 sum |x|)."""
    g = _gen(seed)
    mant = torch.randint(1 << 23, 1 << 24, (n,), generator=g).double()
    expo = torch.randint(-2, 3, (n,), generator=g).double()
    sign = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).double()
    x = (sign * mant * torch.pow(torch.tensor(2.0, dtype=torch.float64), expo - 23)).float()
    return x, float(x.double().sum()), float(x.double().abs().sum())


def sum_bound(d: int, mag: float, ref: float) -> float:
    """|got - ref64| <= (depth 2^-24 sum|x| + 2^-24 |ref64|) (1 + 2^-10): derived in the module docstring."""
    return (d * U * mag + U * abs(ref)) * (1 + 2.0 ** -10)


# ------------------------------------------------------------------------------------------ sizes and probe positions
def _n4_list(max_blocks: int) -> list[int]:
    s = {0, 1, 255, 256, 257, 896}
    def around(v):
        s.update((v - 1, v, v + 1))
    around(3 * THREADS + 1)  # 769: thread 0 passes `tid + 768 < n4`, its first unrolled trip
    around(CHUNK)            # 1024: thread 255 passes it, the block's chunk is full; 1025: a second block
    for k in range(1, 10):   # partial counts 1..9 on the production grid (every np & 3), trips on a capped one
        s.add((k - 1) * CHUNK + 517)
    step = max_blocks * CHUNK
    if 3 * step * 4 <= (1 << 20):  # a capped grid: the trips are in reach of a small tensor
        around(step)                 # the cap binds from step + 1 on: a second trip, clean-up only
        around(step + 3 * THREADS + 1)  # a second unrolled trip
        s.add(step + 896)            # a second trip that is partly clean-up
        around(step + CHUNK)
        around(2 * step)             # every block two trips; 2 step + 1: a third
        around(2 * step + 3 * THREADS + 1)
        s.add(2 * step + 896)
        around(3 * step)
    return sorted(v for v in s if v >= 0)


@functools.lru_cache(maxsize=None)
def interesting_n(max_blocks: int = CAP) -> tuple[int, ...]:
    """The sizes at which `coverage` changes shape (see _n4_list), each n4 crossed with n & 3 in 0..3."""
    return tuple(sorted({4 * n4 + r for n4 in _n4_list(max_blocks) for r in range(4)} - {0}))


def probe_positions(n: int, max_blocks: int = CAP, limit: int = 64) -> list[int]:
    """First and last element of every loop region of coverage(n, max_blocks): per trip the unrolled slots and the
    clean-up turns (so also the last element of each trip and the vector one thread past the last full-unroll
    thread), block borders, and the n & 3 tail."""
    c = coverage(n, max_blocks)
    pos = set()
    if c.n4:
        key = (c.vec_trip * 2 + c.vec_region) * UNROLL + c.vec_slot
        for k in np.unique(key):
            v = np.nonzero(key == k)[0]
            pos.update((4 * int(v[0]), 4 * int(v[-1]) + 3))
        for k in np.unique(c.vec_trip):  # the last element of the trip and its first clean-up vector
            v = np.nonzero(c.vec_trip == k)[0]
            pos.add(4 * int(v[-1]) + 3)
            cl = np.nonzero((c.vec_trip == k) & (c.vec_region == CLEANUP))[0]
            if cl.size:
                pos.update((4 * int(cl[0]) + 1, 4 * int(cl[0]) - 1))
        for v in (CHUNK - 1, CHUNK, c.step - 1, c.step):
            if 0 <= v < c.n4:
                pos.add(4 * v + 2)
    pos.update(range(c.n4 * 4, n))
    pos = sorted(p for p in pos if 0 <= p < n)
    if len(pos) > limit:
        keep = set(pos[:: (len(pos) + limit - 1) // limit]) | set(range(c.n4 * 4, n)) | {pos[-1]}
        pos = sorted(keep)
    return pos


def region_table(sizes, max_blocks: int = CAP) -> str:
    """The loop regions per size as a markdown table (profiles/r22_reduce_scan_tests/README.md)."""
    rows = ["| n | cap | blocks | trips | unrolled vectors per trip | clean-up vectors per trip | tail | np & 3 | depth |",
            "|---|---|---|---|---|---|---|---|---|"]
    for n in sizes:
        c = coverage(n, max_blocks)
        un = [c.regions.get(("unrolled", t), 0) for t in range(c.trips)]
        cl = [c.regions.get(("cleanup", t), 0) for t in range(c.trips)]
        rows.append(f"| {n} | {max_blocks} | {c.nb} | {c.trips} | {un} | {cl} | {n & 3} | {c.np_tail} | {c.depth} |")
    return "\n".join(rows)


# ------------------------------------------------------------------------------------------ assertion functions
def bits(v) -> int:
    a = np.asarray(v)
    return int(a.view(np.uint32 if a.dtype == np.float32 else np.int32))


def same_bits(got, want, dtype=np.float32) -> bool:
    return bits(np.asarray(got, dtype=dtype)) == bits(np.asarray(want, dtype=dtype))


def check_exact_size(run, n: int, max_blocks: int | None):
    """Sum, min and max in float32 and int32 and the dot, on the exact and the weighted family: bit-equal to the truth."""
    cap = CAP if max_blocks is None else max_blocks
    for fam, family in (("exact", exact_family), ("weighted", weighted_family)):
        for dtype, nd in ((torch.float32, np.float32), (torch.int32, np.int32)):
            x, total = family(n, dtype=dtype)
            if dtype is torch.float32:
                assert_order_free(x, n, cap)
            for op, want in (("sum", total), ("min", int(x.min())), ("max", int(x.max()))):
                got = run(op, x, None, max_blocks)
                assert same_bits(got, want, nd), (fam, op, str(dtype), n, max_blocks, got, want)
        a, _ = family(n)
        b = dot_partner(n)
        assert_order_free(a, n, cap, b)
        want = int((a.long() * b.long()).sum())
        for p, q in ((a, b), (b, a)):
            got = run("dot", p, q, max_blocks)
            assert same_bits(got, want), (fam, "dot", n, max_blocks, got, want)


PLANT = {"sum": (0.0, 1.0), "min": (2.0, 1.0), "max": (-2.0, -1.0), "dot": (0.0, 3.0)}  # background, planted value
PLANT_I32 = {"sum": (0, 1), "min": (7, 3), "max": (-7, -3)}


def check_probes(run, n: int, max_blocks: int | None, positions=None):
    """One planted element per run at every probe position: the sum is exactly 1, min and max exactly the planted
    value (float32 and int32); the dot with the probe in a against ones in b and the reverse is the planted 3."""
    cap = CAP if max_blocks is None else max_blocks
    ones = torch.ones(n)
    for p in (probe_positions(n, cap) if positions is None else positions):
        for op in OPS:
            for table, dtype, nd in ((PLANT, torch.float32, np.float32), (PLANT_I32, torch.int32, np.int32)):
                bg, val = table[op]
                x = torch.full((n,), bg, dtype=dtype)
                x[p] = val
                got = run(op, x, None, max_blocks)
                assert same_bits(got, val, nd), (op, str(dtype), n, max_blocks, p, got)
        a = torch.zeros(n)
        a[p] = PLANT["dot"][1]
        for u, v in ((a, ones), (ones, a)):
            got = run("dot", u, v, max_blocks)
            assert same_bits(got, PLANT["dot"][1]), ("dot", n, max_blocks, p, got)


def check_specials(run, n: int, max_blocks: int | None, cpu_sum=None):
    """NaN, inf, -0.0, wrapping and identity-valued inputs at the probe positions of size n (documented behaviour of
    ops.reduce / ops.dot)."""
    cap = CAP if max_blocks is None else max_blocks
    nan, inf = float("nan"), float("inf")
    pos = probe_positions(n, cap, limit=24)
    base, _ = weighted_family(n)
    for p in pos:  # min and max skip a NaN wherever it stands, and do not lose its neighbours in the same float4
        x = base.clone()
        x[p] = nan
        keep = torch.ones(n, dtype=torch.bool)
        keep[p] = False
        q = (p & ~3) + ((p + 1) & 3) if (p & ~3) + 3 < n else p  # a neighbour in p's vector carries the extreme
        if q != p:
            x[q] = -1000.0
        assert same_bits(run("min", x, None, max_blocks), float(x[keep].min())), ("min skips NaN", n, max_blocks, p)
        if q != p:
            x[q] = 1000.0
        assert same_bits(run("max", x, None, max_blocks), float(x[keep].max())), ("max skips NaN", n, max_blocks, p)
        x = base.clone()
        x[p] = nan
        assert np.isnan(run("sum", x, None, max_blocks)), ("sum hands on NaN", n, max_blocks, p)
        x[p] = inf
        assert same_bits(run("sum", x, None, max_blocks), inf), ("sum hands on inf", n, max_blocks, p)
        x[pos[0] if p != pos[0] else pos[-1]] = -inf
        if len(pos) > 1:
            assert np.isnan(run("sum", x, None, max_blocks)), ("+inf + -inf", n, max_blocks, p)
        y = torch.ones(n)
        x = base.clone()
        x[p] = nan
        assert np.isnan(run("dot", x, y, max_blocks)) and np.isnan(run("dot", y, x, max_blocks)), ("dot NaN", n, p)
    # a NaN alone in a block (a one-element input) and all-NaN inputs give the identities
    for m in sorted({1, 3, n}):
        x = torch.full((m,), nan)
        assert same_bits(run("min", x, None, max_blocks), inf), ("all-NaN min", m)
        assert same_bits(run("max", x, None, max_blocks), -inf), ("all-NaN max", m)
        z = torch.full((m,), -0.0)
        assert same_bits(run("sum", z, None, max_blocks), 0.0), ("sum of -0.0 is +0.0", m)
        assert same_bits(run("dot", z, torch.ones(m), max_blocks), 0.0), ("dot of -0.0 is +0.0", m)
    # int32: sums wrap mod 2^32; identity-valued inputs survive
    g = _gen(7)
    xi = torch.randint(1 << 28, (1 << 30), (max(n, 64),), generator=g, dtype=torch.int64).to(torch.int32)
    assert int(xi.long().sum()) > I32_MAX
    want = np.int64(int(xi.long().sum())).astype(np.int32)
    assert same_bits(run("sum", xi, None, max_blocks), want, np.int32), ("int32 wrap", n, max_blocks)
    if cpu_sum is not None:
        assert same_bits(cpu_sum(xi), want, np.int32), "the CPU path wraps the same way"
    assert same_bits(run("max", torch.full((n,), I32_MIN, dtype=torch.int32), None, max_blocks), I32_MIN, np.int32)
    assert same_bits(run("min", torch.full((n,), I32_MAX, dtype=torch.int32), None, max_blocks), I32_MAX, np.int32)


def check_empty(run, max_blocks: int | None):
    """numel() == 0: the identities, bit for bit."""
    e, ei = torch.zeros(0), torch.zeros(0, dtype=torch.int32)
    inf = float("inf")
    for op, want, wi in (("sum", 0.0, 0), ("min", inf, I32_MAX), ("max", -inf, I32_MIN)):
        assert same_bits(run(op, e, None, max_blocks), want), (op, "empty float32")
        assert same_bits(run(op, ei, None, max_blocks), wi, np.int32), (op, "empty int32")
    assert same_bits(run("dot", e, e, max_blocks), 0.0)


# The plan the GPU tests follow (test_gpu_reduce_scan.py) and the CPU tests replay on the model and its mutants:
# max_blocks None is the production entry (ops.reduce / ops.dot on the GPU), a number the capped C entry.
ROUTES = (None, 1, 3, 7)
PROBE_CASES = ((4 * 900 + 3, None),                 # one block: unrolled and clean-up threads, a 3-element tail
               (4 * (4 * CHUNK + 300) + 2, None),   # five blocks, the last one partial; np = 5
               (4 * (7 * CHUNK + 900) + 1, 7))      # capped at 7 blocks: a second trip, partly clean-up; np = 7
SPECIAL_CASES = ((4 * 900 + 3, None), (4 * (3 * CHUNK + 900) + 2, 3))
BIG_N = ((1 << 26) + 4096 * 5 + 3,                  # the production grid's second trip (five blocks, unrolled)
         (1 << 26) + 4096 * 5 + 4 * 900 + 2)        # the same with a sixth block partly in the clean-up loop


def rejecting_checks(run, only=None) -> set[str]:
    """Which of the GPU tests' assertion groups (all, or those named in `only`) reject `run`."""
    groups = {
        "exact": lambda: [check_exact_size(run, n, mb) for mb in ROUTES for n in interesting_n(CAP if mb is None else mb)],
        "probes": lambda: [check_probes(run, n, mb) for n, mb in PROBE_CASES],
        "specials": lambda: [check_specials(run, n, mb) for n, mb in SPECIAL_CASES],
        "empty": lambda: [check_empty(run, mb) for mb in ROUTES],
    }
    out = set()
    for name, fn in groups.items():
        if only is not None and name not in only:
            continue
        try:
            fn()
        except AssertionError:
            out.add(name)
    return out


# ------------------------------------------------------------------------------------------ scan families and sizes
def scan_sizes(extra_tiles=()) -> list[int]:
    sizes = []
    for k in (0, 1, 2, 5):
        for r in (1, 2, 3, 4, 5, TILE - 3, TILE - 2, TILE - 1) + ((0,) if k else ()):
            sizes.append(TILE * k + r)
    return sizes + [TILE * t for t in extra_tiles]


def _scan_order_free(ref: torch.Tensor):
    """Every prefix stays below 2^22 in magnitude, so any difference of two prefixes (every partial sum the scan forms
    over a contiguous range) plus a small init is exact; the look-back adds tile aggregates in any grouping, so the
    sum of their magnitudes stays below 2^22 too."""
    if ref.numel():
        ends = torch.cat([ref[TILE - 1::TILE], ref[-1:]])
        aggs = torch.diff(ends, prepend=ends.new_zeros(1))
        assert int(ref.abs().max()) < 2 ** 22 and int(aggs.abs().sum()) < 2 ** 22


def scan_exact_family(n: int, seed: int = 3):
    """Integers in [-8, 8], balanced: (x, int64 inclusive prefixes); exact in every order (_scan_order_free)."""
    x, _ = exact_family(n, seed)
    ref = torch.cumsum(x.long(), 0)
    _scan_order_free(ref)
    return x, ref


def scan_weighted_family(n: int, seed: int = 0):
    """The weighted family as a scan input: a row written at the wrong offset changes its values."""
    x, _ = weighted_family(n, seed)
    ref = torch.cumsum(x.long(), 0)
    _scan_order_free(ref)
    return x, ref


def scan_truth(ref_incl: torch.Tensor, exclusive: bool, init: float | None) -> torch.Tensor:
    ref = torch.cat([ref_incl.new_zeros(1), ref_incl[:-1]]) if exclusive and ref_incl.numel() else ref_incl
    return (ref + (int(init) if init is not None else 0)).float()


def scan_bound(x: torch.Tensor) -> np.ndarray:
    """scan_depth(i, n) 2^-24 sum_{j <= i} |x_j| (1 + 2^-10) for every i."""
    n = x.numel()
    return scan_depth(np.arange(n), n) * U * torch.cumsum(x.double().abs(), 0).numpy() * (1 + 2.0 ** -10)
