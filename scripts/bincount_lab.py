"""Histogram lab: ops.bincount / ops.histc / ops.histogram against the torch calls they replace, ops.unique with counts
and the copy floor, in one process on one MI355X.

n = 2^28 samples. Rows: int32 bincount for uniform samples over bin counts in the three regimes (all bins in one block's
LDS up to 24576 bins; LDS over bin ranges up to 64 * 24576; global atomics above) and the four distributions (uniform,
equal = every sample in one bin, sorted, zipf) at 256 bins, at the first bin count past each switch, at the last of the
ranged regime and at 2^21 bins; uint8 bincount at 256 bins; float32 histc and explicit edges; int32 and float32 weights. Bars: torch.bincount (torch.histc; bucketize + bincount for edges) and, for int32 samples,
ops.unique(return_counts=True). Floor = ops.copy_ moving as many bytes as the op must read (half of them read, half
written). Every group is timed with device events: warm-ups, then interleaved repetitions (ours, torch, floor, unique,
ours, ...); the table shows the median and the minimum in ms. Every timed output of ours is checked before the row is
printed: exactly against torch.bincount of the bins the definitions give (int32 weights: int64 sums, wrapped; float32
weights: to 1e-5 of an fp64 sum). Whether the torch bar computed the same counts is reported beside it: torch.histc
counts in float32, which stops at 2^24 per bin.

    python scripts/bincount_lab.py [--n N] [--reps R] [--warmup W] [--out FILE]
"""
import argparse
import math
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402

LDS_BINS, RANGED_BINS = ops.vector.HIST_LDS_BINS, ops.vector.HIST_RANGED_BINS


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


def _bins(dist, n, nb, dev):
    u = ops.rand_uniform_(torch.empty(n, device=dev), 13000, 0.0, 1.0)
    if dist == "zipf":
        b = torch.exp(u * math.log(nb + 1.0)).long() - 1
    else:
        b = (u * nb).long()
    b.clamp_(0, nb - 1)
    if dist == "equal":
        b.fill_(nb // 2)
    elif dist == "sorted":
        b = torch.sort(b).values
    return b


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    n = a.n
    src = torch.empty(n + 4096, device=dev)  # copy floor buffers: up to 8n bytes moved
    dst = torch.empty_like(src)
    first_global = RANGED_BINS + 1
    rows = [("bincount", "i32", nb, "uniform", "none")
            for nb in (256, 4096, LDS_BINS, LDS_BINS + 1, 4 * LDS_BINS, 16 * LDS_BINS, 1 << 20, RANGED_BINS, first_global,
                       1 << 21, 1 << 24)]
    rows += [("bincount", "i32", nb, d, "none") for nb in (256, LDS_BINS + 1, RANGED_BINS, first_global, 1 << 21)
             for d in ("equal", "sorted", "zipf")]
    rows += [("bincount", "u8", 256, d, "none") for d in ("uniform", "equal", "sorted", "zipf")]
    rows += [("histc", "f32", nb, d, "none") for nb in (256, LDS_BINS + 1, 1 << 20, first_global) for d in ("uniform", "equal")]
    rows += [("edges", "f32", nb, d, "none") for nb in (64, 8192) for d in ("uniform", "equal")]
    rows += [("bincount", "i32", nb, "uniform", w) for w in ("i32", "f32") for nb in (256, 1 << 21)]
    lines = [f"bincount_lab: n = {n} samples, {a.reps} interleaved reps after {a.warmup} warm-ups, "
             f"{torch.cuda.get_device_name(0)}",
             "| op | samples | bins | dist | weights | ours ms (med / min) | torch ms (med / min) | torch / ours | "
             "floor ms (copy_, same bytes) | ours / floor | ops.unique ms |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for mode, dtype, nb, dist, wkind in rows:
        b = _bins(dist, n, nb, dev)
        w = None
        if wkind != "none":
            wf = ops.rand_uniform_(torch.empty(n, device=dev), 14000, 0.0, 1.0)
            w = wf if wkind == "f32" else (wf * 1000.0).int()
        edges = None
        if dtype == "f32":
            x = (b.float() + 0.5) / float(nb)
        else:
            x = b.to(torch.uint8 if dtype == "u8" else torch.int32)
        if mode == "bincount":
            ours = lambda: ops.bincount(x, nb, w)  # noqa: E731
            bar = lambda: torch.bincount(x, weights=w, minlength=nb)  # noqa: E731
        elif mode == "histc":
            ours = lambda: ops.histc(x, nb, 0.0, 1.0)  # noqa: E731
            bar = lambda: torch.histc(x, nb, 0.0, 1.0)  # noqa: E731
        else:
            edges = torch.linspace(0.0, 1.0, nb + 1, device=dev)
            ours = lambda: ops.histogram(x, edges)  # noqa: E731
            bar = lambda: torch.bincount((torch.bucketize(x, edges, right=True) - 1).clamp_(0, nb - 1), minlength=nb)  # noqa: E731
        got, ref = ours(), bar()
        if wkind == "f32":
            want = torch.zeros(nb, dtype=torch.float64, device=dev).index_add_(0, b, w.double())
            same = bool(((got.double() - want).abs() <= 1e-5 * want.abs().clamp_min(1.0)).all())
            bar_same = bool(((ref.double() - want).abs() <= 1e-5 * want.abs().clamp_min(1.0)).all())
        elif wkind == "i32":
            want = torch.zeros(nb, dtype=torch.int64, device=dev).index_add_(0, b, w.long())
            same = torch.equal(got.long(), ((want + 2**31) % 2**32) - 2**31)
            bar_same = torch.equal(ref.long(), want)
        else:
            # f32 samples sit at bin centres, where the definitions of ops.histc / ops.histogram give bin b
            want = torch.bincount(b, minlength=nb)
            same = torch.equal(got.long(), want)
            bar_same = torch.equal(ref.long(), want)
        note = "" if bar_same else f" torch result differs (largest count {float(ref.max()):.0f}, exact {int(want.max())})"
        del got, ref, want, b
        ok = ok and same
        m = (x.numel() * x.element_size() + (4 * n if w is not None else 0)) // 8  # floats copied: same bytes moved
        fns = {"ours": ours, "torch": bar, "floor": lambda: ops.copy_(dst[:m], src[:m])}
        if dtype == "i32" and wkind == "none":
            fns["unique"] = lambda: ops.unique(x, return_counts=True)
        t = _time_groups(fns, a.reps, a.warmup)
        med = {k_: statistics.median(v_) for k_, v_ in t.items()}
        mn = {k_: min(v_) for k_, v_ in t.items()}
        slower = med["ours"] > med["torch"]
        ratio = f"{med['torch'] / med['ours']:.2f}x"
        uniq = f"{med['unique']:.3f}" if "unique" in med else "-"
        lines.append(f"| {mode} | {dtype} | {nb} | {dist} | {wkind} | {med['ours']:.3f} / {mn['ours']:.3f} | "
                     f"{med['torch']:.3f} / {mn['torch']:.3f} | {'**' + ratio + ' (slower)**' if slower else ratio} | "
                     f"{med['floor']:.3f} | {med['ours'] / med['floor']:.2f}x | {uniq} |" + ("" if same else " MISMATCH") + note)
        print(lines[-1], flush=True)
        del x, w, edges
    lines.append(f"outputs match the oracles: {ok}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
