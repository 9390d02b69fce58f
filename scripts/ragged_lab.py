"""Ragged segment reduction lab: ops.segment_reduce against torch.segment_reduce, against the route until now
(ops.reduce_by_key on segment ids expanded from the offsets) and against the copy floor, in one process on one MI355X.

Cases at N elements (2^28 by default), data and offsets from the "ragged" workload (whole numbers, so float32 sums are
exact wherever a segment's magnitude stays below 2^24): equal segments of mean length 1 / 4 / 100 / 10^5, one segment,
uniformly drawn borders of mean length 100 (some segments empty), power-law rows of mean length 100 (the SpMV matrices'
row lengths), and S = 4 N (most segments empty). Columns:
  ours    ops.segment_reduce(x, offsets, op)
  torch   torch.segment_reduce(x, op, offsets=offsets) (float32 only; int32 rows show n/a)
  by key  ops.reduce_by_key(ids, x, op) with ids[i] = the segment of element i, expanded BEFORE the timed window (the
          expansion is not counted); valid only where no segment is empty (its output drops them) and where the
          offsets cover all elements: n/a elsewhere
  floor   ops.copy_ of the same bytes (the elements and the offsets read once, one result per segment written)
Every cell is timed with device events: warm-ups, then interleaved repetitions; the tables show the median and the
minimum in ms. A call whose first run takes more than --slow-ms is timed over 2 repetitions only (torch.segment_reduce
gives one thread a whole segment). Before a case is timed our output is compared with torch's (exactly where the
workload is exact, else within terms * 2^-23 * sum|x| per segment; float64 prefix differences stand in where torch's call
raises, which the row then says) and with the by-key route's. A ratio below 1 (ours slower) is printed in bold.

    python scripts/ragged_lab.py [--n N] [--reps R] [--warmup W] [--slow-ms MS] [--out FILE]
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


def _once(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _time_interleaved(fns, reps, warmup, slow_ms):
    """Interleaved device-event timings of the callables in fns: {name: [ms, ...]}; a slow call gets 2 repetitions"""
    first = {k: _once(f) for k, f in fns.items()}  # the first run also loads the code objects: never reported
    left = {k: (2 if first[k] > slow_ms else reps) for k in fns}
    for _ in range(max(warmup - 1, 0)):
        for k, f in fns.items():
            if first[k] <= slow_ms:
                f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for r in range(reps):
        for k, f in fns.items():
            if r < left[k]:
                ms[k].append(_once(f))
    return ms


def _cell(t):
    return f"{statistics.median(t):.3f} / {min(t):.3f}"


def _ratio(num, den):
    r = num / den
    return f"**{r:.2f}x**" if r < 1.0 else f"{r:.2f}x"


class Lab:
    def __init__(self, n, reps, warmup, slow_ms, dev):
        self.n, self.reps, self.warmup, self.slow_ms, self.dev = n, reps, warmup, slow_ms, dev
        self.ok, self.lines = True, []
        self.src = self.dst = None

    def say(self, s):
        self.lines.append(s)
        print(s, flush=True)

    def floor(self, nbytes):
        m = max(1, -(-nbytes // 8))
        if self.src is None or self.src.numel() < m:
            self.src = self.dst = None
            self.src = torch.empty(m, device=self.dev)
            self.dst = torch.empty_like(self.src)
        return lambda: ops.copy_(self.dst[:m], self.src[:m])

    def case(self, label, mean_len, dist, dtype, op):
        w = build_workload("ragged", Context(device=self.dev), n=self.n, mean_len=mean_len, dist=dist, op=op, dtype=dtype)
        x, off, s = w.x, w.offsets, w.segments()
        lens = (off[1:] - off[:-1]).long()
        fns = {"ours": w.step}
        w.step()
        torch.cuda.synchronize()  # an error of ours shows here, not in torch's call
        ours = w.out
        same, note = True, ""
        if dtype == "f32":
            try:
                ref = w.torch_step()
                torch.cuda.synchronize()
                fns["torch"] = w.torch_step
            except RuntimeError as e:  # torch refuses some segment counts: the cell says so, the check falls back
                ref, note = None, " torch.segment_reduce raised: " + str(e).splitlines()[0]
                if op == "sum":
                    c = torch.cat([torch.zeros(1, device=self.dev, dtype=torch.float64), torch.cumsum(x.double(), 0)])
                    ref = (c[off[1:].long()] - c[off[:-1].long()]).float()
                    del c
            if ref is not None and w.exact:
                same = torch.equal(ours, ref)
            elif ref is not None:
                c = torch.cat([torch.zeros(1, device=self.dev, dtype=torch.float64), torch.cumsum(x.abs().double(), 0)])
                mag = c[off[1:].long()] - c[off[:-1].long()]
                same = bool(((ours - ref).abs() <= lens * 2.0 ** -23 * mag).all())
                del c, mag
            del ref
        by_key = int(lens.min()) > 0 and int(off[0]) == 0 and int(off[-1]) == self.n
        if by_key:
            ids = torch.repeat_interleave(torch.arange(s, device=self.dev, dtype=torch.int32), lens)
            out_keys, out = torch.empty_like(ids), torch.empty_like(x)
            _, agg, num = ops.reduce_by_key(ids, x, op, out_keys=out_keys, out=out)
            same = same and int(num) == s and (torch.equal(agg[:s], ours) if w.exact else
                                               bool(torch.allclose(agg[:s], ours, rtol=1e-4, atol=1e-2)))
            fns["by key"] = lambda: ops.reduce_by_key(ids, x, op, out_keys=out_keys, out=out)
        del lens
        fns["floor"] = self.floor(int(w.work_per_step()))
        self.ok = self.ok and same
        t = _time_interleaved(fns, self.reps, self.warmup, self.slow_ms)
        med = {k: statistics.median(v) for k, v in t.items()}
        cell = {k: _cell(v) + (f" ({len(v)} reps)" if len(v) != self.reps else "") for k, v in t.items()}
        self.say(f"| {label} | {dtype} {op} | {s} | {cell['ours']} | {cell.get('torch', 'n/a')} | {cell.get('by key', 'n/a')} | "
                 f"{cell['floor']} | " + (_ratio(med["torch"], med["ours"]) if "torch" in med else "n/a") + " | "
                 + (_ratio(med["by key"], med["ours"]) if "by key" in med else "n/a")
                 + f" | {med['ours'] / med['floor']:.2f}x |" + ("" if same else " MISMATCH") + note)

    def run(self):
        self.say("| case | dtype op | segments | ours ms (med / min) | torch ms | by key ms | floor ms (copy_) | torch / ours | "
                 "by key / ours | ours / floor |")
        self.say("|---|---|---|---|---|---|---|---|---|---|")
        n = self.n
        cases = [("equal, length 1", 1, "equal"), ("equal, length 4", 4, "equal"), ("equal, length 100", 100, "equal"),
                 ("equal, length 10^5", 1e5, "equal"), ("one segment", n, "equal"), ("uniform borders, mean 100", 100, "uniform"),
                 ("power-law rows, mean 100", 100, "powerlaw"), ("S = 4 N, mostly empty", 1, "empty")]
        for label, mean_len, dist in cases:
            self.case(label, mean_len, dist, "f32", "sum")
        for dtype, op in (("f32", "min"), ("i32", "sum"), ("i32", "max")):
            self.case("equal, length 100", 100, "equal", dtype, op)
            self.case("one segment", n, "equal", dtype, op)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=float, default=float(1 << 28))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slow-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args(argv)
    lab = Lab(int(a.n), a.reps, a.warmup, a.slow_ms, torch.device("cuda", 0))
    lab.say(f"ragged_lab: {int(a.n)} elements, {a.reps} interleaved reps after {a.warmup} warm-ups, "
            f"{torch.cuda.get_device_name(0)}")
    lab.say("")
    lab.run()
    lab.say("")
    lab.say(f"outputs agree with torch and with the by-key route: {lab.ok}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lab.lines) + "\n")
    return 0 if lab.ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
