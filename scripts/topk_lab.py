"""Top-k lab: the radix select against torch.topk, against sort-and-slice and against the copy floor, in one process on
one MI355X.

n = 2^28 float32 and int32 keys (1 GiB); keys uniform, all equal, and already sorted (ascending); k in {1, 64, 1024,
2^16, 2^20, 2^24, n/2}; sorted=True and sorted=False; the largest are asked for. Columns:
  select   ops.topk(x, k, method="select")             the radix-select kernels (csrc/kernels/topk.hip)
  torch    torch.topk(x, k, largest, sorted)           the vendor bar (its choice among ties is unspecified)
  sort     ops.topk(x, k, method="sort")               the route there was before: ops.sort(x, descending=True) sliced
  floor    ops.copy_ moving as many bytes as the select route reads and writes: five reads of the keys (four histogram
           passes and the gather), 8 bytes per survivor, and for sorted=True the survivor sort's traffic (4 + 4 * 16
           bytes per survivor); a copy of m floats moves 8m bytes
Every cell is timed with device events: warm-ups, then interleaved repetitions (select, torch, sort, floor, select,
...); the table shows the median and the minimum in ms. Before a cell is timed, the select and the sort route's
outputs are compared bit for bit with the first k entries of torch.sort(stable=True) (for sorted=False re-ordered by
index), and torch.topk's sorted values with the same entries.

    python scripts/topk_lab.py [--n N] [--reps R] [--warmup W] [--dtypes f32,i32] [--dists uniform,equal,sorted]
                               [--ks 1,64,...] [--out FILE]
    python scripts/topk_lab.py --one-call [--n N] [--k K]   one warm-up and one call, for a kernel trace
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402


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


def _bytes(n, k, sorted_):
    return 5 * 4 * n + 8 * k + ((4 + 4 * 16) * k if sorted_ and k > 1 else 0)


def _make(dtype, dist, n, dev):
    if dtype == "f32":
        x = ops.rand_uniform_(torch.empty(n, device=dev), 12000, -1.0, 1.0)
    else:
        g = torch.Generator(device=dev).manual_seed(12000)
        x = torch.randint(-2**31, 2**31, (n,), device=dev, generator=g, dtype=torch.int64).int()
    if dist == "equal":
        x.fill_(0.5 if dtype == "f32" else 1)
    elif dist == "sorted":
        x = torch.sort(x).values
    return x


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtypes", default="f32,i32")
    ap.add_argument("--dists", default="uniform,equal,sorted")
    ap.add_argument("--ks", default=None, help="comma-separated k values (default: the issue's seven)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--one-call", action="store_true", help="one warm-up and one select call at --k, nothing else")
    ap.add_argument("--k", type=int, default=1024)
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    n = a.n
    if a.one_call:
        x = _make("f32", "uniform", n, dev)
        for _ in range(2):
            v, i = ops.topk(x, a.k, method="select")
            kv = ops.kth_value(x, a.k, largest=True)
            torch.cuda.synchronize()
        ops.scan_check(dev)
        print(f"one call: n = {n}, k = {a.k}, k-th value {kv.item()!r}, last of top-k {v[-1].item()!r}")
        return 0
    ks = [int(s) for s in a.ks.split(",")] if a.ks else [1, 64, 1024, 1 << 16, 1 << 20, 1 << 24, n // 2]
    ks = [k for k in ks if 1 <= k <= n]
    m_max = max(1, -(-_bytes(n, max(ks), True) // 8))
    src = torch.empty(m_max + 4096, device=dev)
    dst = torch.empty_like(src)
    lines = [f"topk_lab: n = {n} keys ({4 * n / 2**30:.2f} GiB), largest=True, {a.reps} interleaved reps after {a.warmup} "
             f"warm-ups, {torch.cuda.get_device_name(0)}",
             "| keys | data | k | sorted | select ms (med / min) | torch.topk ms (med / min) | sort route ms (med / min) | "
             "floor ms (copy_, same bytes) | torch / select | sort route / select | select / floor |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    ok = True
    for dtype in a.dtypes.split(","):
        for dist in a.dists.split(","):
            x = _make(dtype, dist, n, dev)
            ref = torch.sort(x, stable=True, descending=True)
            ref_v, ref_i = ref.values, ref.indices.int()
            del ref
            for k in ks:
                for sorted_ in (True, False):
                    rv, ri = ref_v[:k], ref_i[:k]
                    if not sorted_:
                        ri, o = torch.sort(ri)
                        rv = rv[o]
                        del o
                    sel = lambda: ops.topk(x, k, sorted=sorted_, method="select")  # noqa: E731
                    srt = lambda: ops.topk(x, k, sorted=sorted_, method="sort")  # noqa: E731
                    bar = lambda: torch.topk(x, k, largest=True, sorted=sorted_)  # noqa: E731
                    same = True
                    for f in (sel, srt):
                        v, i = f()
                        same = same and torch.equal(i, ri) and torch.equal(v.view(torch.int32), rv.view(torch.int32))
                        del v, i
                    fns = {"select": sel, "torch": bar, "sort": srt}
                    try:
                        tv = bar().values
                        if sorted_:
                            same = same and torch.equal(tv, rv)
                        del tv
                    except RuntimeError as e:  # a k torch.topk does not take: the column stays empty
                        print(f"torch.topk failed at k = {k}: {str(e).splitlines()[0]}", flush=True)
                        del fns["torch"]
                    ok = ok and same
                    del rv, ri
                    m = max(1, -(-_bytes(n, k, sorted_) // 8))
                    fns["floor"] = lambda: ops.copy_(dst[:m], src[:m])  # noqa: E731
                    t = _time_interleaved(fns, a.reps, a.warmup)
                    med = {k_: statistics.median(v) for k_, v in t.items()}
                    mn = {k_: min(v) for k_, v in t.items()}
                    tor = f"{med['torch']:.3f} / {mn['torch']:.3f}" if "torch" in med else "n/a"
                    rat = f"{med['torch'] / med['select']:.2f}x" if "torch" in med else "n/a"
                    lines.append(f"| {dtype} | {dist} | {k} | {sorted_} | {med['select']:.3f} / {mn['select']:.3f} | {tor} | "
                                 f"{med['sort']:.3f} / {mn['sort']:.3f} | {med['floor']:.3f} | {rat} | "
                                 f"{med['sort'] / med['select']:.2f}x | {med['select'] / med['floor']:.2f}x |"
                                 + ("" if same else " MISMATCH"))
                    print(lines[-1], flush=True)
            del x, ref_v, ref_i
    ops.scan_check(dev)
    lines.append(f"outputs identical to the stable sort's prefix: {ok}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
