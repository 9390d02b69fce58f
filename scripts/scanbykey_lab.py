"""Scan-by-key lab: ours against the torch composition it replaces, the copy floor, the plain scan and reduce-by-key,
in one process on one MI355X.

n = 2^28 int32 keys (1 GiB) with geometric run lengths of mean 1 (all distinct), 4, 100, 10^5 and all equal:
  sum f32    ops.scan_by_key(k, v, "sum")   bar: unique_consecutive(return_inverse, return_counts) + cumsum - gathered base
  sum i32    the same with int32 values
  positions  ops.run_positions(k)           bar: unique_consecutive + arange - starts[inv]
Every group is timed with device events: warm-ups, then interleaved repetitions (ours, torch, floor, scan, reduce by
key, ours, ...); the table shows the median and the minimum in ms. Floor = ops.copy_ moving the bytes ours must move
once: 12 per element (keys, values, output), 8 for positions. scan = ops.scan on n float32 (8 bytes per element);
reduce by key = ops.reduce_by_key on the same keys and values (ops.run_length_encode for positions). Every timed output
is checked before the table is printed: int32 sums and positions exactly, float32 sums to 1e-5 of an fp64 reference.
Each row is followed by the share of our three kernels in the device time of our call (torch.profiler kernel times):
with all keys equal the lead kernel rewrites the whole output, the case a single-pass variant would remove.

    python scripts/scanbykey_lab.py [--n N] [--reps R] [--warmup W] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402

MEANS = [("1", 1.0), ("4", 4.0), ("100", 100.0), ("1e5", 1e5), ("all equal", 0.0)]
KERNELS = ("scanbykey_tile_kernel", "scanbykey_carry_kernel", "scanbykey_lead_kernel")


def _time_groups(fns, reps, warmup):
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


def _kernel_times(fn, reps=3):
    """Device time in us per call of each of our three kernels in `reps` calls of fn, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        tot = {k: 0.0 for k in KERNELS}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None)
            t = getattr(e, "cuda_time_total", 0.0) if t is None else t
            for tag in tot:
                if tag in e.key:
                    tot[tag] += t
        return {k: v / reps for k, v in tot.items()} if sum(tot.values()) > 0 else None
    except Exception as exc:  # a profiler that is not available leaves the table without these lines
        print(f"(kernel shares not measured: {exc})")
        return None


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="sum f32,sum i32,positions")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    n = a.n
    modes = a.modes.split(",")
    src = torch.empty(3 * n // 2 + 4096, device=dev)  # copy floor buffers: up to 12n bytes moved (6n read, 6n written)
    dst = torch.empty_like(src)
    xs = ops.rand_uniform_(torch.empty(n, device=dev), 12000, 0.0, 1.0)  # the plain scan's input
    lines = [f"scanbykey_lab: n = {n} keys ({4 * n / 2**30:.2f} GiB), {a.reps} interleaved reps after {a.warmup} warm-ups, "
             f"{torch.cuda.get_device_name(0)}",
             "| mode | mean run | runs | ours ms (med / min) | torch ms (med / min) | torch / ours | floor ms (copy_, same bytes) "
             "| ours / floor | ops.scan ms | reduce_by_key ms |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for label, mean in MEANS:
        u = ops.rand_uniform_(torch.empty(n, device=dev), 10000, 0.0, 1.0)
        keys = torch.cumsum(u < (1.0 / mean if mean else 0.0), 0).int()
        vf = ops.rand_uniform_(u, 11000, 0.0, 1.0)
        vi = (vf * 1000.0).int()
        del u
        _, inv, cnt = torch.unique_consecutive(keys, return_inverse=True, return_counts=True)
        k = cnt.numel()
        base_idx = (torch.cumsum(cnt, 0) - cnt)[inv]  # the index of the first element of every element's run
        del inv, cnt
        for mode in modes:
            if mode == "positions":
                ours = lambda: ops.run_positions(keys)  # noqa: E731

                def bar():
                    _, i2, c2 = torch.unique_consecutive(keys, return_inverse=True, return_counts=True)
                    return (torch.arange(n, device=dev) - (torch.cumsum(c2, 0) - c2)[i2]).int()

                other = lambda: ops.run_length_encode(keys)  # noqa: E731
                same = torch.equal(ours().long(), torch.arange(n, device=dev) - base_idx)
                moved = 8 * n
            else:
                v = vf if mode == "sum f32" else vi
                ours = lambda: ops.scan_by_key(keys, v, "sum")  # noqa: E731

                def bar():
                    _, i2, c2 = torch.unique_consecutive(keys, return_inverse=True, return_counts=True)
                    c = torch.cumsum(v, 0, dtype=v.dtype)
                    return c - (c - v)[torch.cumsum(c2, 0) - c2][i2]

                other = lambda: ops.reduce_by_key(keys, v, "sum")  # noqa: E731
                got = ours()
                if v.dtype == torch.int32:
                    c = torch.cumsum(v, 0, dtype=torch.int64)
                    ref = c - (c - v)[base_idx]
                    same = torch.equal(got.long(), ((ref + 2**31) % 2**32) - 2**31)
                else:
                    c = torch.cumsum(v, 0, dtype=torch.float64)
                    ref = c - (c - v)[base_idx]
                    same = bool(((got.double() - ref).abs() <= 1e-5 * ref.abs().clamp_min(1.0)).all())
                del got, c, ref
                moved = 12 * n
            ok = ok and same
            m = moved // 8
            floor = lambda: ops.copy_(dst[:m], src[:m])  # noqa: E731
            scan = lambda: ops.scan(xs)  # noqa: E731
            t = _time_groups({"ours": ours, "torch": bar, "floor": floor, "scan": scan, "other": other}, a.reps, a.warmup)
            med = {k_: statistics.median(v_) for k_, v_ in t.items()}
            mn = {k_: min(v_) for k_, v_ in t.items()}
            slower = med["ours"] > med["torch"]
            ratio = f"{med['torch'] / med['ours']:.2f}x"
            lines.append(f"| {mode} | {label} | {k} | {med['ours']:.3f} / {mn['ours']:.3f} | "
                         f"{med['torch']:.3f} / {mn['torch']:.3f} | {'**' + ratio + ' (slower)**' if slower else ratio} | "
                         f"{med['floor']:.3f} | {med['ours'] / med['floor']:.2f}x | {med['scan']:.3f} | {med['other']:.3f} |"
                         + ("" if same else " MISMATCH"))
            print(lines[-1], flush=True)
            kt = _kernel_times(ours)
            if kt is not None:
                tot = sum(kt.values())
                parts = ", ".join(f"{name.split('_')[1]} {kt[name] / 1e3:.3f} ms ({100 * kt[name] / tot:.1f}%)" for name in KERNELS)
                lines.append(f"|   kernels ({mode}, {label}) | | | {parts}; sum {tot / 1e3:.3f} ms | | | | | | |")
                print(lines[-1], flush=True)
        del keys, vf, vi, base_idx
    ops.scan_check(dev)
    lines.append(f"outputs match the references: {ok}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
