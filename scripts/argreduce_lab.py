"""argmin / argmax lab: ops.arg_reduce and ops.segment_arg_reduce against torch, against the route until now (ops.topk
with k = 1) and against the plain reductions of the same data, in one process on one MI355X. float32 and int32, op max;
data and offsets from the "argreduce" workload (float32: quarter steps of a normal sample, so extrema repeat).

  flat      N elements (2^28): ops.arg_reduce(x, "max") and ops.argmax(x) (no value written) against torch.argmax(x),
            ops.topk(x, 1) (a four-pass radix select, a gather and a sort of one survivor: the route until now) and
            ops.reduce(x, "max") (the value alone), beside ops.copy_ of the same bytes.
  dim       the shapes of the README's reduce-along-a-dimension row: ops.arg_reduce(x, "max", dim) against
            torch.max(x, dim), ops.topk(x, 1, dim=dim) where it takes the shape (n/a elsewhere) and
            ops.reduce(x, "max", dim=dim), the same routes with 4-byte partials.
  segments  N elements with equal lengths 1 / 4 / 100 / 10^5, one segment, uniform borders and power-law rows of mean
            100: ops.segment_arg_reduce(x, offsets, "max") against ops.segment_reduce(x, offsets, "max"), the floor of
            the same scheme with 4-byte partials (torch has no arg form over ragged segments).
Every cell is timed with device events: warm-ups, then interleaved repetitions; the tables show the median and the
minimum in ms. Before a case is timed its outputs are checked on the device: the value equals the plain reduction's, the
element at the returned position is that value, the position is not behind torch's (ties: ours is the first) and equals
the top-1 position. A ratio below 1 (ours slower) is printed in bold.

    python scripts/argreduce_lab.py [--n N] [--reps R] [--warmup W] [--only flat,dim,segments] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402
from parallel_c_programs_amd.models.workloads import build_workload  # noqa: E402
from parallel_c_programs_amd.parallel.dist import Context  # noqa: E402

DIM_SHAPES = [((1 << 20, 32), 1), ((1 << 16, 512), 1), ((16384, 4096), 1), ((1024, 32768), 1), ((8, 1 << 24), 1),
              ((4096, 4096), 0), ((1 << 20, 64), 0), ((64, 1024, 1024), 1)]


def _once(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _time_interleaved(fns, reps, warmup):
    """Interleaved device-event timings of the callables in fns: {name: [ms, ...]}; the first run of each (it loads the
    code objects) and the warm-ups are not reported."""
    for _ in range(max(warmup, 1)):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ms[k].append(_once(f))
    return ms


def _cell(t):
    return f"{statistics.median(t):.3f} / {min(t):.3f}"


def _ratio(num, den):
    r = num / den
    return f"**{r:.2f}x**" if r < 1.0 else f"{r:.2f}x"


class Lab:
    def __init__(self, n, reps, warmup, dev):
        self.n, self.reps, self.warmup, self.dev = n, reps, warmup, dev
        self.ok, self.lines = True, []
        self.src = self.dst = None

    def say(self, s):
        self.lines.append(s)
        print(s, flush=True)

    def check(self, cond, what):
        if not bool(cond):
            self.ok = False
            self.say(f"MISMATCH: {what}")

    def floor(self, nbytes):
        m = max(1, -(-nbytes // 8))
        if self.src is None or self.src.numel() < m:
            self.src = self.dst = None
            self.src = torch.empty(m, device=self.dev)
            self.dst = torch.empty_like(self.src)
        return lambda: ops.copy_(self.dst[:m], self.src[:m])

    def row(self, label, dtype, t, order, against):
        """One table row: the cells of `order`, then the ratios other / ours for `against`, then ours / floor."""
        med = {k: statistics.median(v) for k, v in t.items()}
        cells = " | ".join(_cell(t[k]) if k in t else "n/a" for k in order)
        ratios = " | ".join(_ratio(med[k], med["ours"]) if k in med else "n/a" for k in against)
        self.say(f"| {label} | {dtype} | {cells} | {ratios} | {med['ours'] / med['floor']:.2f}x |")

    def flat(self, dtype):
        w = build_workload("argreduce", Context(device=self.dev), form="flat", op="max", dtype=dtype, n=self.n)
        x = w.x
        v, i = ops.arg_reduce(x, "max")
        ti, (tv, tk) = torch.argmax(x), ops.topk(x, 1)
        self.check(v == ops.reduce(x, "max") and x[i.long()] == v, f"flat {dtype}: value")
        self.check(i <= ti and i == tk[0] and i == ops.argmax(x), f"flat {dtype}: position")
        fns = {"ours": lambda: ops.arg_reduce(x, "max"), "argmax": lambda: ops.argmax(x), "torch": lambda: torch.argmax(x),
               "topk": lambda: ops.topk(x, 1), "reduce": lambda: ops.reduce(x, "max"), "floor": self.floor(4 * x.numel())}
        self.row(f"flat, {x.numel()}", dtype, _time_interleaved(fns, self.reps, self.warmup),
                 ["ours", "argmax", "torch", "topk", "reduce", "floor"], ["torch", "topk", "reduce"])

    def dim(self, shape, d, dtype):
        outer, n, inner = int(torch.Size(shape[:d]).numel()), shape[d], int(torch.Size(shape[d + 1:]).numel())
        w = build_workload("argreduce", Context(device=self.dev), form="dim", op="max", dtype=dtype, outer=outer, n=n, inner=inner)
        x = w.x.view(shape)
        v, i = ops.arg_reduce(x, "max", dim=d)
        tv, ti = torch.max(x, d)
        self.check(torch.equal(v, tv) and torch.equal(v, ops.reduce(x, "max", dim=d)), f"dim {shape} {dtype}: values")
        self.check(torch.equal(x.gather(d, i.long().unsqueeze(d)).squeeze(d), v) and bool((i <= ti).all()), f"dim {shape} {dtype}: positions")
        fns = {"ours": lambda: ops.arg_reduce(x, "max", dim=d), "torch": lambda: torch.max(x, d)}
        try:
            kv, ki = ops.topk(x, 1, dim=d)
            torch.cuda.synchronize()
            self.check(torch.equal(ki.squeeze(d), i), f"dim {shape} {dtype}: top-1 position")
            fns["topk"] = lambda: ops.topk(x, 1, dim=d)
        except (ValueError, RuntimeError):
            pass
        fns["reduce"] = lambda: ops.reduce(x, "max", dim=d)
        fns["floor"] = self.floor(4 * x.numel())
        route = ops.vector._axis_route("reduce", outer, n, inner)
        self.row(f"{list(shape)} dim {d} ({route})", dtype, _time_interleaved(fns, self.reps, self.warmup),
                 ["ours", "torch", "topk", "reduce", "floor"], ["torch", "topk", "reduce"])

    def segments(self, label, mean_len, dist, dtype):
        w = build_workload("argreduce", Context(device=self.dev), form="segments", op="max", dtype=dtype, n=self.n,
                           mean_len=mean_len, dist=dist)
        x, off = w.x, w.offsets
        v, i = ops.segment_arg_reduce(x, off, "max")
        self.check(torch.equal(v, ops.segment_reduce(x, off, "max")), f"segments {label} {dtype}: values")
        full = i >= 0
        self.check(torch.equal(x[i[full].long()], v[full]) and torch.equal(full, off[1:] > off[:-1])
                   and bool(((i >= off[:-1]) & (i < off[1:]) | ~full).all()), f"segments {label} {dtype}: positions")
        del full
        fns = {"ours": lambda: ops.segment_arg_reduce(x, off, "max"), "argmax": lambda: ops.segment_argmax(x, off),
               "reduce": lambda: ops.segment_reduce(x, off, "max"), "floor": self.floor(int(w.work_per_step()))}
        t = _time_interleaved(fns, self.reps, self.warmup)
        med = {k: statistics.median(u) for k, u in t.items()}
        self.say(f"| {label} | {dtype} | {off.numel() - 1} | {_cell(t['ours'])} | {_cell(t['argmax'])} | {_cell(t['reduce'])} | "
                 f"{_cell(t['floor'])} | {_ratio(med['reduce'], med['ours'])} | {med['ours'] / med['floor']:.2f}x |")

    def run(self, only):
        if "flat" in only:
            self.say("| case | dtype | ours ms (med / min) | indices only (ops.argmax) | torch.argmax | ops.topk(x, 1) | ops.reduce | "
                     "floor (copy_) | torch / ours | topk / ours | reduce / ours | ours / floor |")
            self.say("|---|---|---|---|---|---|---|---|---|---|---|---|")
            for dtype in ("f32", "i32"):
                self.flat(dtype)
            self.say("")
        if "dim" in only:
            self.say("| shape, dim (default route) | dtype | ours ms (med / min) | torch.max(x, dim) | ops.topk(x, 1, dim) | "
                     "ops.reduce(dim) | floor (copy_) | torch / ours | topk / ours | reduce / ours | ours / floor |")
            self.say("|---|---|---|---|---|---|---|---|---|---|---|")
            for shape, d in DIM_SHAPES:
                for dtype in ("f32", "i32"):
                    self.dim(shape, d, dtype)
            self.say("")
        if "segments" in only:
            self.say("| case | dtype | segments | ours ms (med / min) | indices only | ops.segment_reduce | floor (copy_) | "
                     "segment_reduce / ours | ours / floor |")
            self.say("|---|---|---|---|---|---|---|---|---|")
            n = self.n
            for label, mean_len, dist in [("equal, length 1", 1, "equal"), ("equal, length 4", 4, "equal"),
                                          ("equal, length 100", 100, "equal"), ("equal, length 10^5", 1e5, "equal"),
                                          ("one segment", n, "equal"), ("uniform borders, mean 100", 100, "uniform"),
                                          ("power-law rows, mean 100", 100, "powerlaw")]:
                for dtype in ("f32", "i32"):
                    self.segments(label, mean_len, dist, dtype)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=float, default=float(1 << 28))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="flat,dim,segments")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args(argv)
    lab = Lab(int(a.n), a.reps, a.warmup, torch.device("cuda", 0))
    lab.say(f"argreduce_lab: {int(a.n)} elements (flat, segments), {a.reps} interleaved reps after {a.warmup} warm-ups, "
            f"{torch.cuda.get_device_name(0)}")
    lab.say("")
    try:
        lab.run(a.only.split(","))
    finally:
        lab.say("")
        lab.say(f"outputs agree with the plain reductions, with torch and with the top-1 route: {lab.ok}")
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("\n".join(lab.lines) + "\n")
    return 0 if lab.ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
