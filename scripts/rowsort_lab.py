"""Row-wise sort lab: ops.sort / ops.topk with dim=-1 against torch, against the Python loop over the 1-D ops and
against the copy floor, and the A/B behind every route constant of ops/vector.py, in one process on one MI355X.

Sections (--sections sort,topk,ab):
  sort  shapes [2^20, 32], [2^16, 512], [2^14, 4096], [4096, 16384], [1024, 32768], [8, 2^24]; keys (ops.sort_keys) and
        keys + indices (ops.sort); f32 (multiples of 1/64, ties in every row) and i32 (full range). Columns: ours (the
        default route, named), torch.sort(x, dim=-1, stable=True), the Python loop over ops.sort_keys / ops.sort per row
        (at most 64 rows, n/a above), and ops.copy_ of the bytes read and written once.
  topk  shapes [1, 131072], [64, 32768], [512, 131072], [4096, 4096], [2^16, 512]; k in {1, 8, 64, 1024} where k <=
        cols; f32, largest, sorted. Columns: ours (default route, named), torch.topk(x, k, dim=-1), the loop over
        ops.topk per row (at most 64 rows), the copy floor.
  ab    the two routes either side of every border, same data: wave vs block over cols around ROWSORT_WAVE_COLS; loop
        vs global over rows at cols = 32768 and over cols at rows in {2, 8}; select vs sortkeep over k / cols at cols in {2048, 16384}; select vs loop
        over cols at rows in {1, 8}.
Every cell is timed with device events: warm-ups, then interleaved repetitions; the tables show the median and the
minimum in ms. Before a cell is timed our outputs are compared bit for bit with torch.sort(dim=-1, stable=True).

    python scripts/rowsort_lab.py [--sections sort,topk,ab] [--reps R] [--warmup W] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402
from parallel_c_programs_amd.ops import vector as V  # noqa: E402

LOOP_MAX_ROWS = 64  # the Python loop column is timed up to here


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


def _make(dtype, rows, cols, dev):
    g = torch.Generator(device=dev).manual_seed(16000)
    if dtype == "f32":
        return torch.round(torch.randn(rows, cols, device=dev, generator=g) * 64) / 64 + 0.0  # (+ 0.0: no -0.0 in the keys)
    return torch.randint(-2**31, 2**31, (rows, cols), device=dev, generator=g, dtype=torch.int64).int()


def _cell(t):
    return f"{statistics.median(t):.3f} / {min(t):.3f}"


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Lab:
    def __init__(self, reps, warmup, dev):
        self.reps, self.warmup, self.dev, self.ok, self.lines = reps, warmup, dev, True, []
        self.src = self.dst = None

    def say(self, s):
        self.lines.append(s)
        print(s, flush=True)

    def floor(self, nbytes):
        m = max(1, -(-nbytes // 8))
        if self.src is None or self.src.numel() < m:
            self.src = torch.empty(m, device=self.dev)
            self.dst = torch.empty_like(self.src)
        return lambda: ops.copy_(self.dst[:m], self.src[:m])

    def time(self, fns):
        t = _time_interleaved(fns, self.reps, self.warmup)
        return {k: statistics.median(v) for k, v in t.items()}, {k: _cell(v) for k, v in t.items()}

    # ------------------------------------------------------------ sort
    def sort(self):
        self.say("| keys | shape | mode | route | ours ms (med / min) | torch.sort ms | loop over rows ms | floor ms (copy_) | "
                 "torch / ours | loop / ours | ours / floor |")
        self.say("|---|---|---|---|---|---|---|---|---|---|---|")
        for rows, cols in ((1 << 20, 32), (1 << 16, 512), (1 << 14, 4096), (4096, 16384), (1024, 32768), (8, 1 << 24)):
            for dtype in ("f32", "i32"):
                x = _make(dtype, rows, cols, self.dev)
                ref = torch.sort(x, dim=-1, stable=True)
                for mode in ("keys", "keys+idx"):
                    if mode == "keys":
                        ours = lambda: ops.sort_keys(x, dim=-1)  # noqa: E731
                        loop = lambda: [ops.sort_keys(r) for r in x]  # noqa: E731
                        same = _same(ours(), ref.values)
                    else:
                        ours = lambda: ops.sort(x, dim=-1)  # noqa: E731
                        loop = lambda: [ops.sort(r) for r in x]  # noqa: E731
                        v, i = ours()
                        same = _same(v, ref.values) and _same(i, ref.indices.int())
                        del v, i
                    self.ok = self.ok and same
                    fns = {"ours": ours, "torch": lambda: torch.sort(x, dim=-1, stable=True),
                           "floor": self.floor(x.numel() * (8 if mode == "keys" else 12))}
                    if rows <= LOOP_MAX_ROWS:
                        fns["loop"] = loop
                    med, cell = self.time(fns)
                    route = V._sort_route(None, rows, cols, "lab")
                    self.say(f"| {dtype} | [{rows}, {cols}] | {mode} | {route} | {cell['ours']} | {cell['torch']} | "
                             f"{cell.get('loop', 'n/a')} | {cell['floor']} | {med['torch'] / med['ours']:.2f}x | "
                             + (f"{med['loop'] / med['ours']:.2f}x" if "loop" in med else "n/a")
                             + f" | {med['ours'] / med['floor']:.2f}x |" + ("" if same else " MISMATCH"))
                del x, ref

    # ------------------------------------------------------------ top-k
    def topk(self):
        self.say("| shape | k | route | ours ms (med / min) | torch.topk ms | loop over rows ms | floor ms (copy_) | "
                 "torch / ours | loop / ours | ours / floor |")
        self.say("|---|---|---|---|---|---|---|---|---|---|")
        for rows, cols in ((1, 131072), (64, 32768), (512, 131072), (4096, 4096), (1 << 16, 512)):
            x = _make("f32", rows, cols, self.dev)
            ref = torch.sort(x, dim=-1, stable=True, descending=True)
            for k in (1, 8, 64, 1024):
                if k > cols:
                    continue
                ours = lambda: ops.topk(x, k, dim=-1)  # noqa: E731
                v, i = ours()
                same = _same(v, ref.values[:, :k]) and _same(i, ref.indices[:, :k].int())
                del v, i
                self.ok = self.ok and same
                fns = {"ours": ours, "torch": lambda: torch.topk(x, k, dim=-1),
                       "floor": self.floor(4 * x.numel() + 8 * rows * k)}
                if rows <= LOOP_MAX_ROWS:
                    fns["loop"] = lambda: [ops.topk(r, k) for r in x]
                med, cell = self.time(fns)
                route = V._topk_route(None, rows, cols, k, "lab")
                self.say(f"| [{rows}, {cols}] | {k} | {route} | {cell['ours']} | {cell['torch']} | {cell.get('loop', 'n/a')} | "
                         f"{cell['floor']} | {med['torch'] / med['ours']:.2f}x | "
                         + (f"{med['loop'] / med['ours']:.2f}x" if "loop" in med else "n/a")
                         + f" | {med['ours'] / med['floor']:.2f}x |" + ("" if same else " MISMATCH"))
            del x, ref

    # ------------------------------------------------------------ route A/Bs
    def _ab(self, title, header, cases):
        """cases: (label, {route name: callable}); the callables return comparable outputs."""
        self.say("")
        self.say(title)
        self.say(header)
        self.say("|---|---|---|---|---|")
        for label, fns in cases():
            outs = {name: f() for name, f in fns.items()}
            (na, oa), (nb, ob) = outs.items()
            oa, ob = (o if isinstance(o, (tuple, list)) else (o,) for o in (oa, ob))
            same = all(_same(s, t) for s, t in zip(oa, ob))
            self.ok = self.ok and same
            del outs, oa, ob
            med, cell = self.time(fns)
            self.say(f"| {label} | {cell[na]} | {cell[nb]} | {med[nb] / med[na]:.2f}x | {na if med[na] <= med[nb] else nb} |"
                     + ("" if same else " MISMATCH"))

    def ab(self):
        dev = self.dev

        def wave_block():
            for cols in (32, 64, 128, 256, 512, 1024):
                for mode in ("keys", "keys+idx"):
                    rows = (1 << 24) // cols
                    x = _make("f32", rows, cols, dev)
                    f = ops.sort_keys if mode == "keys" else ops.sort
                    yield f"[{rows}, {cols}] f32 {mode}", {r: (lambda r=r, x=x, f=f: f(x, dim=-1, route=r)) for r in ("wave", "block")}

        self._ab(f"A/B wave vs block (ROWSORT_WAVE_COLS = {V.ROWSORT_WAVE_COLS})",
                 "| case | wave ms (med / min) | block ms | block / wave | faster |", wave_block)

        def loop_global():
            for rows in (1, 2, 4, 8, 16, 64):
                x = _make("f32", rows, 32768, dev)
                yield f"[{rows}, 32768] f32 keys+idx", {r: (lambda r=r, x=x: ops.sort(x, dim=-1, route=r)) for r in ("loop", "global")}
            for cols in (1 << 20, 1 << 22, 1 << 23, 1 << 24):
                for rows in (2, 8):
                    x = _make("f32", rows, cols, dev)
                    yield f"[{rows}, {cols}] f32 keys+idx", {r: (lambda r=r, x=x: ops.sort(x, dim=-1, route=r)) for r in ("loop", "global")}
                    yield f"[{rows}, {cols}] f32 keys", {r: (lambda r=r, x=x: ops.sort_keys(x, dim=-1, route=r)) for r in ("loop", "global")}

        self._ab(f"A/B loop vs global (ROWSORT_LOOP_MIN_COLS = {V.ROWSORT_LOOP_MIN_COLS}; one row is always loop: the same work)",
                 "| case | loop ms (med / min) | global ms | global / loop | faster |", loop_global)

        def select_sortkeep():
            for cols in (2048, 16384):
                x = _make("f32", (1 << 24) // cols, cols, dev)
                for frac in (1 / 64, 1 / 16, 1 / 8, 1 / 4, 1 / 2, 3 / 4, 1):
                    k = max(1, int(cols * frac))
                    yield (f"[{x.shape[0]}, {cols}] f32 k = {k} ({frac:.3f} cols)",
                           {r: (lambda r=r, x=x, k=k: ops.topk(x, k, dim=-1, route=r)) for r in ("select", "sortkeep")})

        self._ab(f"A/B select vs sortkeep (ROW_TOPK_SORT_FRACTION = {V.ROW_TOPK_SORT_FRACTION})",
                 "| case | select ms (med / min) | sortkeep ms | sortkeep / select | faster |", select_sortkeep)

        def select_loop():
            for rows in (1, 8):
                for cols in (1 << 15, 1 << 17, 1 << 19, 1 << 21, 1 << 23):
                    x = _make("f32", rows, cols, dev)
                    yield (f"[{rows}, {cols}] f32 k = 64",
                           {r: (lambda r=r, x=x: ops.topk(x, 64, dim=-1, route=r)) for r in ("select", "loop")})

        self._ab(f"A/B select vs loop (ROW_TOPK_LOOP_COLS_PER_ROW = {V.ROW_TOPK_LOOP_COLS_PER_ROW})",
                 "| case | select ms (med / min) | loop ms | loop / select | faster |", select_loop)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sections", default="sort,topk,ab")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args(argv)
    lab = Lab(a.reps, a.warmup, torch.device("cuda", 0))
    lab.say(f"rowsort_lab: {a.reps} interleaved reps after {a.warmup} warm-ups, {torch.cuda.get_device_name(0)}")
    for s in a.sections.split(","):
        lab.say("")
        getattr(lab, s)()
    ops.scan_check(lab.dev)
    lab.say("")
    lab.say(f"outputs identical to torch.sort(dim=-1, stable=True) / between the two routes: {lab.ok}")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lab.lines) + "\n")
    return 0 if lab.ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
