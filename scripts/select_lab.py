"""Stream-compaction lab: ours against the torch bar and the copy floor, in one process on one MI355X.

n = 2^28 f32 (1 GiB of payload), keep fractions 0 / 0.01 / 0.5 / 1.0, the three front ends:
  mask   ops.compact(x, mask)            bar: x[mask] (torch.masked_select)
  index  ops.compact_indices(mask)       bar: torch.nonzero(mask)
  where  ops.compact_where(x, "lt", t)   bar: x[x < t]  (t = the keep fraction; x uniform in [0, 1))
Every pair is timed with device events: warm-ups, then interleaved repetitions (ours, bar, ours, bar, ...); the table
shows the median and the minimum in ms. The torch bars synchronise for the size of their result inside the timed
region: that sync is part of what a caller of x[mask] pays. Floor = ops.copy_ moving the same number of bytes as the
select must move (5n + 4k, n + 4k, 4n + 4k), rounded up to whole f32 pairs (a copy of m floats moves 8m bytes).
Every timed output is checked against the bar's, bit for bit, before the table is printed.

    python scripts/select_lab.py [--n N] [--reps R] [--warmup W] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402

KEEPS = [0.0, 0.01, 0.5, 1.0]


def _time_pairs(fns, reps, warmup):
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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    n = a.n
    x = ops.rand_uniform_(torch.empty(n, device=dev), 7000, 0.0, 1.0)
    u = ops.rand_uniform_(torch.empty(n, device=dev), 8000, 0.0, 1.0)
    out_f = torch.empty(n, device=dev)
    out_i = torch.empty(n, device=dev, dtype=torch.int32)
    src = torch.empty(3 * n // 2 + 16, device=dev)  # copy floor buffers: up to 9n bytes moved = 9n/8 floats
    dst = torch.empty_like(src)
    lines = [f"select_lab: n = {n} f32 ({4 * n / 2**30:.2f} GiB payload), {a.reps} interleaved reps after {a.warmup} warm-ups, "
             f"{torch.cuda.get_device_name(0)}",
             "| mode | keep | kept | ours ms (med / min) | torch ms (med / min) | torch / ours | floor ms (copy_, same bytes) | ours / floor | ours GB/s |",
             "|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for mode in ("mask", "index", "where"):
        for keep in KEEPS:
            mask = (u < keep) if mode != "where" else None
            if mode == "mask":
                ours = lambda: ops.compact(x, mask, out=out_f)  # noqa: E731
                bar = lambda: x[mask]  # noqa: E731
            elif mode == "index":
                ours = lambda: ops.compact_indices(mask, out=out_i)  # noqa: E731
                bar = lambda: torch.nonzero(mask)  # noqa: E731
            else:
                ours = lambda: ops.compact_where(x, "lt", keep, out=out_f)  # noqa: E731
                bar = lambda: x[x < keep]  # noqa: E731
            got, count = ours()
            k = int(count.item())
            ref = bar().flatten()
            same = k == ref.numel() and torch.equal(got[:k].view(torch.int32), ref.to(got.dtype).view(torch.int32))
            ok = ok and same
            del ref
            nbytes = {"mask": 5 * n, "index": n, "where": 4 * n}[mode] + 4 * k
            m = max(1, -(-nbytes // 8))
            floor = lambda: ops.copy_(dst[:m], src[:m])  # noqa: E731
            t = _time_pairs({"ours": ours, "torch": bar, "floor": floor}, a.reps, a.warmup)
            med = {k_: statistics.median(v) for k_, v in t.items()}
            mn = {k_: min(v) for k_, v in t.items()}
            lines.append(f"| {mode} | {keep} | {k} | {med['ours']:.3f} / {mn['ours']:.3f} | {med['torch']:.3f} / {mn['torch']:.3f} | "
                         f"{med['torch'] / med['ours']:.2f}x | {med['floor']:.3f} | {med['ours'] / med['floor']:.2f}x | "
                         f"{nbytes / med['ours'] / 1e6:.0f} |" + ("" if same else " MISMATCH"))
            print(lines[-1], flush=True)
    ops.scan_check(dev)
    lines.append(f"outputs bit-identical to torch: {ok}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
