"""Reduce / scan along a dimension lab: ops.reduce / ops.scan with dim= against torch, against the copy floor, against
the composition the column routes replace, and the A/B behind every route constant (AXIS_*) of ops/vector.py, in one
process on one MI355X.

Sections (--sections torch,ab):
  torch  float32 (whole numbers in [-8, 8]); the four calls torch.sum(dim), torch.amax(dim), torch.cumsum(dim) and
         torch.cummax(dim).values on [2^20, 32], [2^16, 512], [2^14, 4096], [1024, 32768], [8, 2^24] and one row of 2^28
         along the last dim; [4096, 4096], [2^20, 64], [64, 2^20] along dim 0; [64, 1024, 1024] along dim 1. Columns: ours
         (the default route, named), torch, ops.copy_ of the same bytes (a reduce reads the input: a copy of half as
         many elements; a scan reads and writes it: a copy of as many), and "other": for dims that are not the last the
         composition x.movedim(dim, -1).contiguous() followed by the row route (and movedim back for a scan); for the
         one row of 2^28 the flat ops.reduce / ops.scan (sums only), which stay the default for flat tensors.
  ab     the two routes either side of every border, same data, reduce (sum) and scan (sum): group against block
         around AXIS_GROUP_N; block against split over rows and row lengths around AXIS_SPLIT_ROWS / AXIS_SPLIT_MIN_N;
         split chunks around AXIS_SPLIT_CHUNK; column against column_split around AXIS_COLUMN_MIN_UNITS (scan) and
         AXIS_COLUMN_MIN_BLOCKS (reduce).
Every cell is timed with device events: warm-ups, then interleaved repetitions; the tables show the median and the
minimum in ms. Before a cell is timed our output is compared with torch's (min / max exactly, sums to 1e-6 relative of
the row's sum of magnitudes) or, in an A/B, between the two routes.

    python scripts/axis_lab.py [--sections torch,ab] [--reps R] [--warmup W] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402
from parallel_c_programs_amd.ops import vector as V  # noqa: E402

CALLS = {  # name: (mode, op, the torch call)
    "sum": ("reduce", "sum", lambda x, d: torch.sum(x, d)),
    "amax": ("reduce", "max", lambda x, d: torch.amax(x, d)),
    "cumsum": ("scan", "sum", lambda x, d: torch.cumsum(x, d)),
    "cummax": ("scan", "max", lambda x, d: torch.cummax(x, d).values),
}


def _time_interleaved(fns, reps, warmup):
    """Interleaved device-event timings of the callables in fns: {name: [ms, ...]}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for name, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return ms


def _cell(t):
    return f"{statistics.median(t):.3f} / {min(t):.3f}"


def _ours(x, mode, op, dim, route=None, chunk=None):
    if mode == "reduce":
        return ops.reduce(x, op, dim=dim, route=route, chunk=chunk)
    return ops.scan(x, dim=dim, op=op, route=route, chunk=chunk)


def _close(a, b, x, dim, op):
    if a.shape != b.shape:
        return False
    if op != "sum":
        return torch.equal(a, b)
    return bool(((a - b).abs() <= 1e-6 * x.abs().sum(dim, keepdim=a.dim() == x.dim()) + 1e-6).all())


class Lab:
    def __init__(self, reps, warmup, dev):
        self.reps, self.warmup, self.dev, self.ok, self.lines = reps, warmup, dev, True, []
        self.src = self.dst = None

    def say(self, s):
        self.lines.append(s)
        print(s, flush=True)

    def make(self, shape):
        g = torch.Generator(device=self.dev).manual_seed(17000)
        return torch.randint(-8, 9, shape, device=self.dev, generator=g, dtype=torch.int64).float()

    def floor(self, nbytes):
        m = max(1, -(-nbytes // 8))
        if self.src is None or self.src.numel() < m:
            self.src = self.dst = None
            self.src = torch.empty(m, device=self.dev)
            self.dst = torch.empty_like(self.src)
        return lambda: ops.copy_(self.dst[:m], self.src[:m])

    def time(self, fns):
        t = _time_interleaved(fns, self.reps, self.warmup)
        return {k: statistics.median(v) for k, v in t.items()}, {k: _cell(v) for k, v in t.items()}

    # ------------------------------------------------------------ against torch
    def torch(self):
        self.say("| shape | dim | call | route | ours ms (med / min) | torch ms | floor ms (copy_) | other ms | torch / ours | "
                 "other / ours | ours / floor |")
        self.say("|---|---|---|---|---|---|---|---|---|---|---|")
        cases = [((1 << 20, 32), -1), ((1 << 16, 512), -1), ((1 << 14, 4096), -1), ((1024, 32768), -1), ((8, 1 << 24), -1),
                 ((1 << 28,), 0), ((4096, 4096), 0), ((1 << 20, 64), 0), ((64, 1 << 20), 0), ((64, 1024, 1024), 1)]
        for shape, dim in cases:
            x = self.make(shape)
            d = dim % x.dim()
            outer, n, inner = int(torch.Size(shape[:d]).numel()), shape[d], int(torch.Size(shape[d + 1:]).numel())
            for name, (mode, op, tcall) in CALLS.items():
                route = V._axis_route(mode, outer, n, inner)
                same = _close(_ours(x, mode, op, dim), tcall(x, dim), x, dim, op)
                self.ok = self.ok and same
                nbytes = 4 * x.numel() * (2 if mode == "scan" else 1)
                fns = {"ours": lambda: _ours(x, mode, op, dim), "torch": lambda: tcall(x, dim), "floor": self.floor(nbytes)}
                if inner > 1 and mode == "reduce":
                    fns["other"] = lambda: _ours(x.movedim(dim, -1).contiguous(), mode, op, -1)
                elif inner > 1:
                    fns["other"] = lambda: _ours(x.movedim(dim, -1).contiguous(), mode, op, -1).movedim(-1, dim).contiguous()
                elif len(shape) == 1 and op == "sum":
                    fns["other"] = (lambda: ops.reduce(x)) if mode == "reduce" else (lambda: ops.scan(x))
                med, cell = self.time(fns)
                self.say(f"| {list(shape)} | {dim} | {name} | {route} | {cell['ours']} | {cell['torch']} | {cell['floor']} | "
                         f"{cell.get('other', 'n/a')} | {med['torch'] / med['ours']:.2f}x | "
                         + (f"{med['other'] / med['ours']:.2f}x" if "other" in med else "n/a")
                         + f" | {med['ours'] / med['floor']:.2f}x |" + ("" if same else " MISMATCH"))
            del x

    # ------------------------------------------------------------ route A/Bs
    def _ab(self, title, cases):
        """cases: (label, x, dim, {column name: (route, chunk)}): both modes, sum"""
        self.say("")
        self.say(title)
        first = True
        for label, x, dim, routes in cases():
            names = list(routes)
            if first:
                self.say("| case | mode | " + " | ".join(f"{r} ms (med / min)" for r in names) + " | faster |")
                self.say("|---|---|" + "---|" * (len(names) + 1))
                first = False
            for mode in ("reduce", "scan"):
                fns = {r: (lambda rc=rc: _ours(x, mode, "sum", dim, *rc)) for r, rc in routes.items()}
                outs = [f() for f in fns.values()]
                same = all(_close(o, outs[0], x, dim, "sum") for o in outs[1:])
                self.ok = self.ok and same
                del outs
                med, cell = self.time(fns)
                self.say(f"| {label} | {mode} | " + " | ".join(cell[r] for r in names) + f" | {min(med, key=med.get)} |"
                         + ("" if same else " MISMATCH"))

    def ab(self):
        def group_block():
            for n in (128, 256, 512, 1024, 2048, 4096):
                yield f"[{(1 << 24) // n}, {n}]", self.make(((1 << 24) // n, n)), -1, {"group": ("group", None), "block": ("block", None)}

        self._ab(f"A/B group vs block (AXIS_GROUP_N = {V.AXIS_GROUP_N})", group_block)

        def block_split():
            for rows in (1, 8, 64, 256, 1024):
                for n in (1 << 15, 1 << 17, 1 << 19, 1 << 20):
                    if rows * n <= 1 << 27:
                        yield f"[{rows}, {n}]", self.make((rows, n)), -1, {"block": ("block", None), "split": ("split", None)}

        self._ab(f"A/B block vs split (AXIS_SPLIT_ROWS = {V.AXIS_SPLIT_ROWS}, AXIS_SPLIT_MIN_N = {V.AXIS_SPLIT_MIN_N})", block_split)

        def split_chunk():
            for shape in ((8, 1 << 24), (1, 1 << 26), (64, 1 << 20)):
                yield f"{list(shape)}", self.make(shape), -1, {f"chunk {c}": ("split", c) for c in (8192, 32768, 131072)}

        self._ab(f"split chunk (AXIS_SPLIT_CHUNK = {V.AXIS_SPLIT_CHUNK})", split_chunk)

        def column_split():
            for shape in ((4096, 4096), (1 << 20, 64), (1024, 1 << 14), (1024, 1 << 15), (1024, 1 << 16), (256, 1 << 18),
                          (32, 1 << 18), (1 << 14, 1 << 12)):
                yield f"{list(shape)} dim 0", self.make(shape), 0, {"column": ("column", None), "column_split": ("column_split", None)}
            yield "[64, 1024, 1024] dim 1", self.make((64, 1024, 1024)), 1, {"column": ("column", None), "column_split": ("column_split", None)}

        self._ab(f"A/B column vs column_split (scan: AXIS_COLUMN_MIN_UNITS = {V.AXIS_COLUMN_MIN_UNITS} threads; reduce: "
                 f"AXIS_COLUMN_MIN_BLOCKS = {V.AXIS_COLUMN_MIN_BLOCKS} blocks of 64 column quads; "
                 f"AXIS_COLUMN_SPLIT_MIN_N = {V.AXIS_COLUMN_SPLIT_MIN_N})", column_split)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", default="torch,ab")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args(argv)
    lab = Lab(a.reps, a.warmup, torch.device("cuda", 0))
    lab.say(f"axis_lab: {a.reps} interleaved reps after {a.warmup} warm-ups, {torch.cuda.get_device_name(0)}")
    for s in a.sections.split(","):
        lab.say("")
        getattr(lab, s)()
    lab.say("")
    lab.say(f"outputs agree with torch / between the routes: {lab.ok}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lab.lines) + "\n")
    return 0 if lab.ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
