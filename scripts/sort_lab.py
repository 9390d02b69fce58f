"""Radix-sort lab: ours against the torch call it replaces and the copy floor, in one process on one MI355X.

n = 2^28 keys (1 GiB), three comparisons on three data sets:
  keys     ops.sort_keys(x)            bar: torch.sort(x).values
  sort     ops.sort(x)                 bar: torch.sort(x, stable=True)           (values + indices)
  argsort  ops.argsort(k, bits=20)     bar: torch.sort(k, stable=True).indices   (int32 keys below 2^20)
  data: uniform f32 in [-1, 1), uniform int32 over the full range (argsort: over [0, 2^20)), and all keys equal (every
  key in one digit bin: the worst case of the per-digit chain and of the LDS counters).
Every triple is timed with device events: warm-ups, then interleaved repetitions (ours, bar, floor, ours, ...); the
table shows the median and the minimum in ms. Floor = ops.copy_ moving the bytes our sort must move: the histogram
read (4n), 8n per pass for the keys (16n with values; an argsort's first pass reads no values and its last writes no
keys) and the 1 KiB per tile and pass of flag reset, rounded up to whole f32 pairs (a copy of m floats moves 8m
bytes). Every timed output is checked against the bar's before the table is printed.

    python scripts/sort_lab.py [--n N] [--reps R] [--warmup W] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402

TILE = 16384


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


def _bytes(n, mode, passes):
    """Bytes our sort moves: histogram read, key (and value) traffic of every pass, flag reset."""
    per_pass = 8 if mode == "keys" else 16
    skipped = {"keys": 0, "sort": 4, "argsort": 8}[mode]  # index modes: no value read in pass 0; argsort: no last key write
    return n * (4 + passes * per_pass - skipped) + passes * 1024 * -(-n // TILE)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    n = a.n
    g = torch.Generator(device=dev).manual_seed(9000)
    data = {
        ("f32", "uniform"): lambda: ops.rand_uniform_(torch.empty(n, device=dev), 9000, -1.0, 1.0),
        ("i32", "uniform"): lambda: torch.randint(-2**31, 2**31, (n,), device=dev, generator=g, dtype=torch.int64).int(),
        ("i32<2^20", "uniform"): lambda: torch.randint(0, 1 << 20, (n,), device=dev, generator=g, dtype=torch.int64).int(),
        ("f32", "all equal"): lambda: torch.full((n,), 0.5, device=dev),
        ("i32<2^20", "all equal"): lambda: torch.full((n,), 77, device=dev, dtype=torch.int32),
    }
    cases = [("keys", "f32", "uniform"), ("keys", "i32", "uniform"), ("keys", "f32", "all equal"),
             ("sort", "f32", "uniform"), ("sort", "i32", "uniform"), ("sort", "f32", "all equal"),
             ("argsort", "i32<2^20", "uniform"), ("argsort", "i32<2^20", "all equal")]
    src = torch.empty(17 * n // 2 + 4096, device=dev)  # copy floor buffers: up to 68n bytes moved = 68n/8 floats
    dst = torch.empty_like(src)
    lines = [f"sort_lab: n = {n} keys ({4 * n / 2**30:.2f} GiB), {a.reps} interleaved reps after {a.warmup} warm-ups, "
             f"{torch.cuda.get_device_name(0)}",
             "| mode | keys | data | passes | ours ms (med / min) | torch ms (med / min) | torch / ours | floor ms (copy_, same bytes) "
             "| ours / floor | ours Gkeys/s |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    last, x = None, None
    for mode, dtype, dist in cases:
        if (dtype, dist) != last:
            del x
            x = data[(dtype, dist)]()
            last = (dtype, dist)
        if mode == "keys":
            passes = 4
            ours = lambda: ops.sort_keys(x)  # noqa: E731
            bar = lambda: torch.sort(x).values  # noqa: E731
            same = torch.equal(ours().view(torch.int32), bar().view(torch.int32))
        elif mode == "sort":
            passes = 4
            ours = lambda: ops.sort(x)  # noqa: E731
            bar = lambda: torch.sort(x, stable=True)  # noqa: E731
            (v, i), r = ours(), bar()
            same = torch.equal(v.view(torch.int32), r.values.view(torch.int32)) and torch.equal(i, r.indices.int())
            del v, i, r
        else:
            passes = 3
            ours = lambda: ops.argsort(x, bits=20)  # noqa: E731
            bar = lambda: torch.sort(x, stable=True).indices  # noqa: E731
            same = torch.equal(ours(), bar().int())
        ok = ok and same
        m = max(1, -(-_bytes(n, mode, passes) // 8))
        floor = lambda: ops.copy_(dst[:m], src[:m])  # noqa: E731
        t = _time_pairs({"ours": ours, "torch": bar, "floor": floor}, a.reps, a.warmup)
        med = {k_: statistics.median(v) for k_, v in t.items()}
        mn = {k_: min(v) for k_, v in t.items()}
        lines.append(f"| {mode} | {dtype} | {dist} | {passes} | {med['ours']:.3f} / {mn['ours']:.3f} | "
                     f"{med['torch']:.3f} / {mn['torch']:.3f} | {med['torch'] / med['ours']:.2f}x | {med['floor']:.3f} | "
                     f"{med['ours'] / med['floor']:.2f}x | {n / med['ours'] / 1e6:.2f} |" + ("" if same else " MISMATCH"))
        print(lines[-1], flush=True)
    ops.scan_check(dev)
    lines.append(f"outputs identical to torch: {ok}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
