"""Run-length encode / reduce-by-key lab: ours against the torch calls it replaces and the copy floor, in one process
on one MI355X.

n = 2^28 keys (1 GiB), int32 keys with geometric run lengths of mean 1 (all distinct), 4, 100, 10^5 and all equal:
  rle      ops.run_length_encode(k)            bar: torch.unique_consecutive(k, return_counts=True)
  sum i32  ops.reduce_by_key(k, v, "sum")      bar: torch.unique_consecutive(k, return_inverse=True) + index_add_
  sum f32  the same with float32 values
  unique   ops.unique(x, return_counts=True)   bar: torch.unique(x, return_counts=True)   (x: n draws from n / mean values)
Every triple is timed with device events: warm-ups, then interleaved repetitions (ours, bar, floor, ours, ...); the
table shows the median and the minimum in ms. Floor = ops.copy_ moving the bytes ours must move: the keys (and values)
once and 8 bytes per run; unique adds the sort's traffic (4n histogram read + 4 passes of 8n). Every timed output is
checked against the bar's before the table is printed (float32 sums to 1e-5 of the fp64 sum). The all-equal rows are
followed by the share of the lead fix-up kernel in the device time of our call (torch.profiler kernel times): that
is the case the chain design is for.

    python scripts/segreduce_lab.py [--n N] [--reps R] [--warmup W] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402

MEANS = [("1", 1.0), ("4", 4.0), ("100", 100.0), ("1e5", 1e5), ("all equal", 0.0)]


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


def _fixup_share(fn, reps=3):
    """Device time of the lead fix-up kernel over that of both segreduce kernels in `reps` calls of fn, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        tot = {"lead_fixup_kernel": 0.0, "segreduce_kernel": 0.0}
        for e in prof.key_averages():
            t = getattr(e, "device_time_total", None)
            t = getattr(e, "cuda_time_total", 0.0) if t is None else t
            for tag in tot:
                if tag in e.key:
                    tot[tag] += t
        both = tot["lead_fixup_kernel"] + tot["segreduce_kernel"]
        return (tot["lead_fixup_kernel"] / both, tot["lead_fixup_kernel"] / reps, both / reps) if both > 0 else None
    except Exception as exc:  # a profiler that is not available leaves the table without this line
        print(f"(fix-up share not measured: {exc})")
        return None


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--modes", default="rle,sum i32,sum f32,unique")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    n = a.n
    modes = a.modes.split(",")
    src = torch.empty(11 * n // 2 + 4096, device=dev)  # copy floor buffers: up to 44n + 8n bytes moved
    dst = torch.empty_like(src)
    lines = [f"segreduce_lab: n = {n} keys ({4 * n / 2**30:.2f} GiB), {a.reps} interleaved reps after {a.warmup} warm-ups, "
             f"{torch.cuda.get_device_name(0)}",
             "| mode | mean run | runs | ours ms (med / min) | torch ms (med / min) | torch / ours | floor ms (copy_, same bytes) "
             "| ours / floor |",
             "|---|---|---|---|---|---|---|---|"]
    ok = True
    for label, mean in MEANS:
        u = ops.rand_uniform_(torch.empty(n, device=dev), 10000, 0.0, 1.0)
        keys = torch.cumsum(u < (1.0 / mean if mean else 0.0), 0).int()
        groups = max(1, int(n / mean)) if mean else 1
        x = (u.double() * groups).long().clamp_(max=groups - 1).int()  # unsorted, about `mean` copies of every value
        vf = ops.rand_uniform_(u, 11000, 0.0, 1.0)
        vi = (vf * 1000.0).int()
        for mode in modes:
            if mode == "rle":
                ours = lambda: ops.run_length_encode(keys)  # noqa: E731
                bar = lambda: torch.unique_consecutive(keys, return_counts=True)  # noqa: E731
                (rk, rc, num), (tk, tc) = ours(), bar()
                k = int(num.item())
                same = k == tk.numel() and torch.equal(rk[:k], tk) and torch.equal(rc[:k].long(), tc)
                moved = 4 * n + 8 * k
                del rk, rc, tk, tc
            elif mode in ("sum i32", "sum f32"):
                v = vi if mode == "sum i32" else vf
                ours = lambda: ops.reduce_by_key(keys, v, "sum")  # noqa: E731

                def bar():
                    tk, inv = torch.unique_consecutive(keys, return_inverse=True)
                    return tk, torch.zeros(tk.numel(), dtype=v.dtype, device=dev).index_add_(0, inv, v)

                (rk, ra, num) = ours()
                k = int(num.item())
                tk, inv = torch.unique_consecutive(keys, return_inverse=True)
                acc = torch.int64 if v.dtype == torch.int32 else torch.float64
                ref = torch.zeros(tk.numel(), dtype=acc, device=dev).index_add_(0, inv, v.to(acc))
                del inv
                same = k == tk.numel() and torch.equal(rk[:k], tk)
                if same and v.dtype == torch.int32:
                    same = torch.equal(ra[:k].long(), ((ref + 2**31) % 2**32) - 2**31)
                elif same:
                    same = bool(((ra[:k].double() - ref).abs() <= 1e-5 * ref.abs().clamp_min(1.0)).all())
                moved = 8 * n + 8 * k
                del rk, ra, tk, ref
            else:
                ours = lambda: ops.unique(x, return_counts=True)  # noqa: E731
                bar = lambda: torch.unique(x, return_counts=True)  # noqa: E731
                (uv, uc), (tv, tc) = ours(), bar()
                k = uv.numel()
                same = k == tv.numel() and torch.equal(uv, tv) and torch.equal(uc.long(), tc)
                moved = (4 + 4 * 8 + 4) * n + 8 * k
                del uv, uc, tv, tc
            ok = ok and same
            m = max(1, -(-moved // 8))
            floor = lambda: ops.copy_(dst[:m], src[:m])  # noqa: E731
            t = _time_pairs({"ours": ours, "torch": bar, "floor": floor}, a.reps, a.warmup)
            med = {k_: statistics.median(v_) for k_, v_ in t.items()}
            mn = {k_: min(v_) for k_, v_ in t.items()}
            slower = med["ours"] > med["torch"]
            ratio = f"{med['torch'] / med['ours']:.2f}x"
            lines.append(f"| {mode} | {label} | {k} | {med['ours']:.3f} / {mn['ours']:.3f} | "
                         f"{med['torch']:.3f} / {mn['torch']:.3f} | {'**' + ratio + ' (slower)**' if slower else ratio} | "
                         f"{med['floor']:.3f} | {med['ours'] / med['floor']:.2f}x |" + ("" if same else " MISMATCH"))
            print(lines[-1], flush=True)
            if mean == 0.0 and mode != "unique":
                share = _fixup_share(ours)
                if share is not None:
                    lines.append(f"|   fix-up kernel share ({mode}, all equal) | | | {share[0] * 100:.1f}% of our device time: "
                                 f"{share[1] / 1e3:.3f} of {share[2] / 1e3:.3f} ms per call | | | | |")
                    print(lines[-1], flush=True)
        del keys, x, vf, vi, u
    ops.scan_check(dev)
    lines.append(f"outputs match torch: {ok}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
