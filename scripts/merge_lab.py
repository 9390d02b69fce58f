"""Merge lab: ops.merge_keys / merge / merge_by_key and ops.searchsorted against what a user calls today, in one
process on one MI355X.

Merge rows: 2^27 + 2^27 keys and 2^28 + 2^20 keys (a small sorted chunk into a big sorted array); float32 and int32;
interleaved, disjoint and all-equal keys. Bars: the project's radix sort of the concatenation (ops.sort_keys / ops.sort /
ops.sort_by_key of torch.cat, the cat included, as a caller pays for it) and torch.sort of the same. Search rows: a
2^28-key haystack with 2^20 and 2^28 needles, in random order and sorted, without and (sorted needles) with
values_sorted=True, which takes the merge route from an eighth as many needles as keys; bar: torch.searchsorted. Floor = ops.copy_ moving as many bytes as the op must move (half read, half
written); the general search is charged its needles and results only.

Every group is timed with device events: warm-ups to settle, then TWO runs of interleaved repetitions (ours, bars, floor,
ours, ...); the table shows the median of each run in ms. Every timed output of ours is checked before its row is printed,
exactly, against the stable torch.sort of the concatenation or torch.searchsorted. The gate line at the end compares
merge_keys with ops.sort_keys(torch.cat(...)) at 2^27 + 2^27 float32 keys: the merge must be faster by more than the
gap between the bar's two runs.

    python scripts/merge_lab.py [--scale K] [--reps R] [--warmup W] [--out FILE]

--scale K divides every size by 2^K (a rehearsal; the published table is --scale 0).
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402


def _time_runs(fns, reps, warmup, runs=2):
    """Interleaved device-event timings: {name: [median ms of run 0, of run 1]}."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(runs):
        ms = {k: [] for k in fns}
        for _ in range(reps):
            for name, f in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                f()
                b.record()
                b.synchronize()
                ms[name].append(a.elapsed_time(b))
        for k, v in ms.items():
            out[k].append(statistics.median(v))
    return out


def _keys(n, dtype, seed, lo, hi, dev):
    if dtype == "f32":
        return ops.rand_uniform_(torch.empty(n, device=dev), seed, lo, hi)
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randint(int(lo * (1 << 31)), int(hi * (1 << 31)), (n,), device=dev, generator=g, dtype=torch.int64).int()


def _pair(na, nb, dtype, dist, dev):
    ra, rb = ((-1.0, 0.0), (0.0, 1.0)) if dist == "disjoint" else ((-1.0, 1.0), (-1.0, 1.0))
    a, b = _keys(na, dtype, 15000, *ra, dev), _keys(nb, dtype, 16000, *rb, dev)
    if dist == "equal":
        a.fill_(1), b.fill_(1)
    return torch.sort(a).values, torch.sort(b).values


def _fmt(t):
    return f"{t[0]:.3f} / {t[1]:.3f}"


def _ratio(bar, ours):
    r = f"{min(bar) / min(ours):.2f}x"
    return f"**{r} (slower)**" if min(ours) > min(bar) else r


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    sh = a.scale
    big, half, chunk = (1 << 28) >> sh, (1 << 27) >> sh, (1 << 20) >> sh
    src = torch.empty(2 * (big + chunk) + 4096, device=dev)  # copy floor buffers: up to 16 bytes per key moved
    dst = torch.empty_like(src)
    lines = [f"merge_lab: sizes / 2^{sh}, two runs of {a.reps} interleaved reps after {a.warmup} warm-ups, "
             f"{torch.cuda.get_device_name(0)}; ms are the medians of run 1 / run 2; ratios use the better run of each",
             "",
             "| op | na + nb | dtype | dist | ours ms | ops.sort of cat ms | sort / ours | torch.sort of cat ms | torch / ours | "
             "floor ms (copy_, same bytes) | ours / floor |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    ok, gate = True, None
    merge_rows = [("keys", half, half, "f32", d) for d in ("interleaved", "disjoint", "equal")]
    merge_rows += [("keys", half, half, "i32", "interleaved"), ("pairs", half, half, "f32", "interleaved"),
                   ("index", half, half, "f32", "interleaved"), ("index", half, half, "i32", "interleaved")]
    merge_rows += [(m, big, chunk, "f32", "interleaved") for m in ("keys", "pairs", "index")]
    for mode, na, nb, dtype, dist in merge_rows:
        x, y = _pair(na, nb, dtype, dist, dev)
        n = na + nb
        vx = torch.arange(na, device=dev, dtype=torch.int32)
        vy = torch.arange(na, n, device=dev, dtype=torch.int32)
        if mode == "keys":
            ours = lambda: (ops.merge_keys(x, y),)  # noqa: E731
            sort = lambda: ops.sort_keys(torch.cat([x, y]))  # noqa: E731
            bar = lambda: torch.sort(torch.cat([x, y])).values  # noqa: E731
        elif mode == "pairs":
            ours = lambda: ops.merge_by_key(x, vx, y, vy)  # noqa: E731
            sort = lambda: ops.sort_by_key(torch.cat([x, y]), torch.cat([vx, vy]))  # noqa: E731
            bar = lambda: torch.sort(torch.cat([x, y]), stable=True)  # noqa: E731
        else:
            ours = lambda: ops.merge(x, y)  # noqa: E731
            sort = lambda: ops.sort(torch.cat([x, y]))  # noqa: E731
            bar = lambda: torch.sort(torch.cat([x, y]), stable=True)  # noqa: E731
        got = ours()
        ref = torch.sort(torch.cat([x, y]), stable=True)
        same = torch.equal(got[0].view(torch.int32), ref.values.view(torch.int32))
        if mode != "keys":
            same = same and torch.equal(got[1], ref.indices.int())
        del got, ref
        ok = ok and same
        m = n * {"keys": 8, "pairs": 16, "index": 12}[mode] // 8
        t = _time_runs({"ours": ours, "sort": sort, "torch": bar, "floor": lambda: ops.copy_(dst[:m], src[:m])},
                       a.reps, a.warmup)
        if (mode, na, nb, dtype, dist) == ("keys", half, half, "f32", "interleaved"):
            gate = (t["ours"], t["sort"])
        lines.append(f"| merge {mode} | {na} + {nb} | {dtype} | {dist} | {_fmt(t['ours'])} | {_fmt(t['sort'])} | "
                     f"{_ratio(t['sort'], t['ours'])} | {_fmt(t['torch'])} | {_ratio(t['torch'], t['ours'])} | "
                     f"{_fmt(t['floor'])} | {min(t['ours']) / min(t['floor']):.2f}x |" + ("" if same else " MISMATCH"))
        print(lines[-1], flush=True)
        del x, y, vx, vy
    head = ["",
            "| search | haystack | needles | order | route | ours ms | torch.searchsorted ms | torch / ours | "
            "floor ms (copy_, same bytes) | ours / floor |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    lines += head
    print("\n".join(head), flush=True)
    hay = torch.sort(_keys(big, "f32", 17000, -1.0, 1.0, dev)).values
    for m_needles in (chunk, big):
        rnd = _keys(m_needles, "f32", 18000, -1.0, 1.0, dev)
        srt = torch.sort(rnd).values
        for order, vals, promise in (("random", rnd, False), ("sorted", srt, False), ("sorted", srt, True)):
            ours = lambda: ops.searchsorted(hay, vals, values_sorted=promise)  # noqa: E731
            bar = lambda: torch.searchsorted(hay, vals)  # noqa: E731
            same = torch.equal(ours(), bar().int())
            ok = ok and same
            moved = 4 * (big + m_needles) + 4 * m_needles if promise and 8 * m_needles >= big else 8 * m_needles
            m = moved // 8
            t = _time_runs({"ours": ours, "torch": bar, "floor": lambda: ops.copy_(dst[:m], src[:m])}, a.reps, a.warmup)
            lines.append(f"| searchsorted | {big} | {m_needles} | {order} | {'values_sorted=True' if promise else 'general'} | "
                         f"{_fmt(t['ours'])} | {_fmt(t['torch'])} | {_ratio(t['torch'], t['ours'])} | {_fmt(t['floor'])} | "
                         f"{min(t['ours']) / min(t['floor']):.2f}x |" + ("" if same else " MISMATCH"))
            print(lines[-1], flush=True)
        del rnd, srt
    lines.append("")
    lines.append(f"outputs match the oracles: {ok}")
    if gate is not None:
        ours, bar = gate
        gap = abs(bar[0] - bar[1])
        passed = min(bar) - max(ours) > gap
        lines.append(f"gate (merge_keys against ops.sort_keys(torch.cat) at {half} + {half} float32 keys): merge {_fmt(ours)} ms, "
                     f"bar {_fmt(bar)} ms, gap between the bar's runs {gap:.3f} ms, margin {min(bar) - max(ours):.3f} ms: "
                     f"{'PASSED' if passed else 'FAILED'}")
        ok = ok and passed
    text = "\n".join(lines)
    print("\n".join(lines[-3:]))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
