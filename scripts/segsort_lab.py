"""Ragged segment sort lab: ops.segment_sort* against the route until now (route="global": two device-wide stable
sorts), against the same composition written in torch, for equal lengths against the row sort on the [S, L] view, and
against the copy floor, in one process on one MI355X.

Cases at N float32 keys (2^28 by default), keys and offsets from the "segsort" workload: equal segments of 4 / 32 / 100 /
4096 / 16384 keys, uniformly drawn borders of mean length 100 (some segments empty), power-law rows of mean length 100,
one segment, and a mix of 100-key segments with 1% of the keys in 65536-key segments (above the in-CU limit). Modes keys
/ index / pairs, and int32 keys alone. Columns:
  ours    ops.segment_sort_keys / segment_sort / segment_sort_by_key (route=None; the 16-byte host sync included)
  global  the same op with route="global"
  torch   a stable torch.sort of the keys, a stable torch.sort of the segment ids (expanded BEFORE the timed window), and
          the gathers that give the same outputs
  row     ops.sort_keys / sort / sort_by_key(dim=-1) on the [S, L] view (equal lengths that divide N only)
  floor   ops.copy_ of the bytes a caller sees move (keys and offsets read once, every output written once)
Every cell is timed with device events: warm-ups, then interleaved repetitions; the tables show the median and the
minimum in ms. Before a case is timed our outputs are compared bit for bit with the global route's. A ratio below 1
(ours slower) is printed in bold.

--grid-ab times the class kernels' fixed grid at 2 / 4 / 8 / 16 / 32 blocks per compute unit (keys + indices).

    python scripts/segsort_lab.py [--n N] [--reps R] [--warmup W] [--modes keys,index,pairs] [--grid-ab] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402
from parallel_c_programs_amd.models.workloads import build_workload  # noqa: E402
from parallel_c_programs_amd.ops import vector as V  # noqa: E402
from parallel_c_programs_amd.parallel.dist import Context  # noqa: E402


def _once(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _time_interleaved(fns, reps, warmup):
    for _ in range(max(warmup, 1)):  # the first run also loads the code objects: never reported
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


def _same(a, b):
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


class Lab:
    def __init__(self, n, reps, warmup, dev):
        self.n, self.reps, self.warmup, self.dev = n, reps, warmup, dev
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

    def workload(self, mean_len, dist, mode, dtype):
        mix = dist == "mix"
        w = build_workload("segsort", Context(device=self.dev), n=self.n, mean_len=100 if mix else mean_len,
                           dist="equal" if mix else dist, mode=mode, dtype=dtype)
        if mix:  # the last 1% of the keys in 65536-key segments
            long_len = 65536
            k = max(1, self.n // 100 // long_len)
            cut = (self.n - k * long_len) // 100 * 100
            head = torch.arange(0, cut + 1, 100, device=self.dev, dtype=torch.int64)
            tail = cut + torch.arange(1, k + 1, device=self.dev, dtype=torch.int64) * ((self.n - cut) // k)
            tail[-1] = self.n
            w.offsets = torch.cat([head, tail]).to(torch.int32).contiguous()
            w.seg_ids = None
        return w

    def case(self, label, mean_len, dist, mode, dtype):
        w = self.workload(mean_len, dist, mode, dtype)
        s = w.segments()
        fns = {"ours": w.step}
        w.step()
        torch.cuda.synchronize()
        ours = w.out
        w.route = "global"
        w.step()
        same = _same(ours, w.out)
        w.out = None

        def run_global():
            w.route = "global"
            w.step()
            w.route = None

        w.route = None
        fns["global"] = run_global
        w.torch_step()  # expands the segment ids

        def run_torch():
            x = w.x
            v, i = torch.sort(x, stable=True, descending=w.descending)
            order = i[torch.sort(w.seg_ids[i], stable=True).indices]
            if mode == "keys":
                return x[order]
            if mode == "index":
                return x[order], order.int()
            return x[order], x[order]

        fns["torch"] = run_torch
        L = int(mean_len)
        # (the row sort's wave kernel launches rows / 4 blocks of 256 threads: 2^26 rows are more threads than a launch takes)
        if dist == "equal" and L <= V.SEGSORT_MAX_LEN and self.n % L == 0 and s == self.n // L and s < 1 << 26:
            x2 = w.x.view(s, L)
            row = {"keys": lambda: ops.sort_keys(x2, dim=-1), "index": lambda: ops.sort(x2, dim=-1),
                   "pairs": lambda: ops.sort_by_key(x2, x2, dim=-1)}[mode]
            ref = [t.view(-1) for t in (row() if mode != "keys" else (row(),))]
            if mode == "index":  # the row sort gives positions within the row
                ref[1] = (ref[1].view(s, L) + torch.arange(s, device=self.dev, dtype=torch.int32)[:, None] * L).view(-1)
            same = same and _same(ours, ref)
            del ref
            fns["row"] = row
        del ours
        fns["floor"] = self.floor(int(w.work_per_step()))
        self.ok = self.ok and same
        t = _time_interleaved(fns, self.reps, self.warmup)
        med = {k: statistics.median(v) for k, v in t.items()}
        cell = {k: _cell(v) for k, v in t.items()}
        self.say(f"| {label} | {dtype} {mode} | {s} | {cell['ours']} | {cell['global']} | {cell['torch']} | "
                 f"{cell.get('row', 'n/a')} | {cell['floor']} | {_ratio(med['global'], med['ours'])} | "
                 f"{_ratio(med['torch'], med['ours'])} | " + (_ratio(med["row"], med["ours"]) if "row" in med else "n/a")
                 + f" | {med['ours'] / med['floor']:.2f}x |" + ("" if same else " MISMATCH"))
        w.out = None
        del w
        torch.cuda.empty_cache()

    CASES = [("equal, length 4", 4, "equal"), ("equal, length 32", 32, "equal"), ("equal, length 100", 100, "equal"),
             ("equal, length 4096", 4096, "equal"), ("equal, length 16384", 16384, "equal"),
             ("uniform borders, mean 100", 100, "uniform"), ("power-law rows, mean 100", 100, "powerlaw"),
             ("one segment", None, "equal"), ("100-key segments, 1% of the keys in 65536-key segments", 100, "mix")]

    def run(self, modes):
        self.say("| case | dtype mode | segments | ours ms (med / min) | global ms | torch ms | row sort ms | floor ms (copy_) | "
                 "global / ours | torch / ours | row / ours | ours / floor |")
        self.say("|---|---|---|---|---|---|---|---|---|---|---|---|")
        for mode in modes:
            for label, mean_len, dist in self.CASES:
                self.case(label, self.n if mean_len is None else mean_len, dist, mode, "f32")
        for label, mean_len, dist in self.CASES:
            self.case(label, self.n if mean_len is None else mean_len, dist, "keys", "i32")

    def grid_ab(self):
        mults = (2, 4, 8, 16, 32)
        self.say("")
        self.say("| case (f32, keys + indices) | " + " | ".join(f"{m} blocks / CU" for m in mults) + " |")
        self.say("|---|" + "---|" * len(mults))
        for label, mean_len, dist in [c for c in self.CASES if c[2] != "mix" and c[1] is not None]:
            w = self.workload(mean_len, dist, "index", "f32")
            fns = {m: (lambda m=m: V._segment_sort(w.x, None, w.offsets, "index", False, None, False, None, None,
                                                   "segment_sort", grid_mult=m)) for m in mults}
            t = _time_interleaved(fns, self.reps, self.warmup)
            self.say(f"| {label} | " + " | ".join(_cell(t[m]) for m in mults) + " |")
            del w
            torch.cuda.empty_cache()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=float, default=float(1 << 28))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default="keys,index,pairs")
    ap.add_argument("--grid-ab", action="store_true", help="only the A/B of the class kernels' blocks per compute unit")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args(argv)
    lab = Lab(int(a.n), a.reps, a.warmup, torch.device("cuda", 0))
    lab.say(f"segsort_lab: {int(a.n)} keys, {a.reps} interleaved reps after {a.warmup} warm-ups, "
            f"{torch.cuda.get_device_name(0)}")
    lab.say("")
    if a.grid_ab:
        lab.grid_ab()
    else:
        lab.run([m for m in a.modes.split(",") if m])
        lab.say("")
        lab.say(f"outputs agree with the global route (and the row sort where it applies): {lab.ok}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lab.lines) + "\n")
    return 0 if lab.ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
