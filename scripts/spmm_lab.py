"""SpMM lab: ops.spmm against the routes a user had until now, in one process on one MI355X.

Candidates, per matrix and width k of the dense block X [n_cols, k]:
  ours    ops.spmm(m, X, out=Y) (csrc/kernels/spmm.hip), at the default item size of the width class and, with
          --items, at every item size given;
  k-spmv  k calls of ops.spmv(m, x_c) on the contiguous columns of X (the transposition is not timed, nor is the
          scatter of the results into Y);
  torch   torch.mm of a torch.sparse_csr_tensor with X;
  floor   ops.copy_ of the compulsory bytes, 8 nnz + 4 k (n_cols + n_rows).
The table also gives the gathered bytes, 4 k nnz, and their rate in ours.

Every candidate is warmed up, then called back to back for a settle period (--settle seconds) before anything is
recorded; the repetitions are interleaved over the candidates and timed with device events; the table shows the median
and the minimum in ms. Before a case is timed ours is checked: a seeded sample of rows against the fp64 product inside
the any-order rounding bound (the spmm workload's check), and every column against the k-spmv route to 1e-4 of the
column's largest entry. A ratio below 1 (ours slower) is printed in bold. Progress lines ("[seconds] what") go to
the standard output between the table rows and are not part of --out.

    python scripts/spmm_lab.py [--cases small,large,banded,uniform] [--k 4,16,64,256] [--items 64,128,256,512,1024]
                               [--reps R] [--warmup W] [--settle S] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402
from parallel_c_programs_amd.models.workloads import SpMM  # noqa: E402
from parallel_c_programs_amd.parallel.dist import Context  # noqa: E402

CASES = {"small": ("powerlaw_csr(1e6, 1e7)", lambda: ops.powerlaw_csr(1_000_000, 10_000_000)),
         "large": ("powerlaw_csr(1e7, 1e8)", lambda: ops.powerlaw_csr(10_000_000, 100_000_000)),
         "banded": ("banded 100000 401 200 100 200 10", lambda: ops.banded_csr(100_000, 401, 200, 100, 200, 10)),
         "uniform": ("uniform, 1e6 rows of 16", None)}
CASE_K = {"small": (4, 16, 64, 256), "large": (4, 16, 64, 256), "banded": (64,), "uniform": (64,)}


def _once(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _time_interleaved(fns, reps, warmup, settle, note=lambda s: None):
    for name, f in fns.items():
        note(f"warm-up and settle: {name}")
        for _ in range(max(warmup, 1)):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < settle:  # settle: clocks and caches at their steady state
            f()
            torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for r in range(reps):
        note(f"repetition {r + 1} of {reps}")
        for k, f in fns.items():
            ms[k].append(_once(f))
    return ms


def _cell(t):
    return f"{statistics.median(t):.3f} / {min(t):.3f}"


def _ratio(num, den):
    r = num / den
    return f"**{r:.2f}x**" if r < 1.0 else f"{r:.2f}x"


class Lab:
    def __init__(self, reps, warmup, settle, dev):
        self.reps, self.warmup, self.settle, self.dev = reps, warmup, settle, dev
        self.ok, self.lines, self.t0 = True, [], time.perf_counter()

    def say(self, s):
        self.lines.append(s)
        print(s, flush=True)

    def note(self, s):
        """Progress (not part of the tables): what the lab is doing, with the seconds since it started."""
        print(f"[{time.perf_counter() - self.t0:7.1f} s] {s}", flush=True)

    def check(self, cond, what):
        if not bool(cond):
            self.ok = False
            self.say(f"MISMATCH: {what}")

    def matrix(self, case):
        label, build = CASES[case]
        self.note(f"building {label}")
        if build is None:
            w = SpMM(Context(device=torch.device("cpu")), n_rows=1_000_000, nnz=16_000_000, k=1, matrix="uniform")
            return label, w.m.to(self.dev)
        return label, build().to(self.dev)

    def case(self, label, m, k, items):
        self.note(f"{label}, k = {k}: operands and the k-spmv result")
        m.plan()
        w = SpMM(Context(device=self.dev), k=k, csr=m)
        x, y = w.x, w.out
        xt = x.t().contiguous()
        ycols = torch.empty(k, m.n_rows, device=self.dev)

        def kspmv():
            for c in range(k):
                ops.spmv(m, xt[c])

        for c in range(k):
            ycols[c] = ops.spmv(m, xt[c])
        default = ops.sparse.spmm_item_nnz(k)
        fns = {}
        for item in [default] + [i for i in items if i != default]:
            self.note(f"check at item size {item}")
            w.item_nnz = item
            m.spmm_plan(item)
            y.fill_(float("nan"))
            w.step()
            chk = w.check()
            self.check(chk["check_passed"], f"{label} k={k} item {item}: fp64 sample, worst err / bound {chk['worst_err_over_bound']:.3f}")
            dev = ((y.t() - ycols).abs().amax(1) / ycols.abs().amax(1).clamp_min(1e-30)).max()
            self.check(dev <= 1e-4, f"{label} k={k} item {item}: against the k-spmv route, {float(dev):.3e}")
            fns["ours" if item == default else f"item {item}"] = (lambda it=item: ops.spmm(m, x, out=y, item_nnz=it))
        fns["k-spmv"] = kspmv
        self.note("torch.mm of the sparse CSR tensor")
        try:
            a = torch.sparse_csr_tensor(m.row_ptr, m.col.long(), m.val, size=(m.n_rows, m.n_cols))
            yt = torch.mm(a, x)
            dev = ((yt - y).abs().amax(0) / yt.abs().amax(0).clamp_min(1e-30)).max()
            self.check(dev <= 1e-4, f"{label} k={k}: against torch.mm, {float(dev):.3e}")
            del yt
            fns["torch"] = lambda: torch.mm(a, x)
        except (RuntimeError, NotImplementedError) as e:
            self.say(f"(torch.mm of a sparse CSR tensor not available for {label} k={k}: {str(e).splitlines()[0][:100]})")
        nbytes = w.compulsory_bytes()
        src = torch.empty(-(-nbytes // 8), device=self.dev)
        dst = torch.empty_like(src)
        fns["floor"] = lambda: ops.copy_(dst, src)
        t = _time_interleaved(fns, self.reps, self.warmup, self.settle, self.note)
        med = {n: statistics.median(v) for n, v in t.items()}
        gathered = 4.0 * k * m.nnz
        cells = " | ".join(_cell(t[n]) if n in t else "n/a" for n in ("ours", "k-spmv", "torch", "floor"))
        self.say(f"| {label} | {k} | {default} | {cells} | {_ratio(med['k-spmv'], med['ours'])} | "
                 f"{_ratio(med['torch'], med['ours']) if 'torch' in med else 'n/a'} | {med['ours'] / med['floor']:.2f}x | "
                 f"{2.0 * m.nnz * k / med['ours'] / 1e6:.0f} | {nbytes / med['ours'] / 1e6:.0f} | {gathered / 1e9:.2f} | "
                 f"{gathered / med['ours'] / 1e6:.0f} |")
        sweep = [(n, v) for n, v in t.items() if n.startswith("item ")]
        if sweep:
            self.sweeps.append(f"| {label} | {k} | ours = {default}: {_cell(t['ours'])} | " +
                               " | ".join(f"{n}: {_cell(v)}" for n, v in sweep) + " |")

    def run(self, cases, ks, items):
        self.sweeps = []
        self.say("| matrix | k | item size | ours ms (med / min) | k x ops.spmv | torch.mm (sparse CSR) | floor (copy_) | "
                 "k-spmv / ours | torch / ours | ours / floor | GFLOP/s | compulsory GB/s | gathered GB | gathered GB/s |")
        self.say("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
        for case in cases:
            label, m = self.matrix(case)
            for k in CASE_K[case]:
                if k in ks:
                    self.case(label, m, k, items if k in (64, 256) else [])
            del m
            torch.cuda.empty_cache()
        if self.sweeps:
            self.say("")
            self.say("Item sizes at k = 64 and 256 (ms, med / min):")
            self.say("")
            for s in self.sweeps:
                self.say(s)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="small,large,banded,uniform")
    ap.add_argument("--k", default="4,16,64,256")
    ap.add_argument("--items", default="64,128,256,512,1024")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settle", type=float, default=0.3)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args(argv)
    lab = Lab(a.reps, a.warmup, a.settle, torch.device("cuda", 0))
    lab.say(f"spmm_lab: {a.reps} interleaved reps after {a.warmup} warm-ups and {a.settle} s of settling per candidate, "
            f"{torch.cuda.get_device_name(0)}")
    lab.say("")
    try:
        lab.run(a.cases.split(","), [int(v) for v in a.k.split(",")], [int(v) for v in a.items.split(",") if v])
    finally:
        lab.say("")
        lab.say(f"ours agrees with the fp64 sample, the k-spmv route and torch: {lab.ok}")
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text("\n".join(lab.lines) + "\n")
    return 0 if lab.ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
