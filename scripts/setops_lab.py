"""Set-operation lab: ops.set_compact / set_compact_by_key against the routes a user has without them, in one process
on one MI355X.

Rows: 2^27 + 2^27 keys; the four ops; float32 and int32; modes keys / index / pairs; dists interleaved (both sides from
one range; float32 draws repeat, int32 draws hardly do), disjoint, identical, ties (eight keys) and equal (one key).
Bars:
  (a) the composition of existing ops, keys mode: per side two ops.searchsorted(values_sorted=True) of its keys in the
      other side (lower and upper bound), ops.run_positions, a comparison in torch and ops.compact; union and symmetric
      difference then ops.merge_keys the two kept parts. The multiset result, bit for bit.
  (b) torch's nearest equivalent, on the duplicate-free int32 interleaved rows only (elsewhere it computes another
      result): torch.isin(assume_unique=True) plus a mask select for intersection and difference, torch.unique of the
      concatenation for union. Nothing for symmetric difference.
  (c) ops.merge_keys (ops.merge / ops.merge_by_key in index / pairs mode) of the same inputs: the same bytes read, the
      same merge, every element written.
  (d) ops.copy_ of the bytes the op moves (inputs read once, kept elements written once; half read, half written).

Every group is timed with device events: warm-ups, then TWO runs of interleaved repetitions (ours, bars, floor, ours,
...); the table shows the median of each run in ms. Every timed output of ours is checked before its row is printed,
exactly, against bar (a)'s formulation computed with torch.searchsorted.

    python scripts/setops_lab.py [--scale K] [--reps R] [--warmup W] [--out FILE] [--quick]

--scale K divides every size by 2^K (a rehearsal; the published table is --scale 0). --quick keeps the keys-mode rows
of the interleaved dist and one row per other mode and dist.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from parallel_c_programs_amd import ops  # noqa: E402

OPS = ["intersection", "union", "difference", "symmetric_difference"]


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


def _pair(n, dtype, dist, dev):
    tdt = torch.float32 if dtype == "f32" else torch.int32
    if dist == "ties":
        g = torch.Generator(device=dev).manual_seed(17000)
        a, b = (torch.randint(0, 8, (n,), device=dev, generator=g).to(tdt) for _ in range(2))
    elif dist == "equal":
        a, b = torch.ones(n, device=dev, dtype=tdt), torch.ones(n, device=dev, dtype=tdt)
    else:
        ra, rb = ((-1.0, 0.0), (0.0, 1.0)) if dist == "disjoint" else ((-1.0, 1.0), (-1.0, 1.0))
        a = _keys(n, dtype, 17000, *ra, dev)
        b = a.clone() if dist == "identical" else _keys(n, dtype, 18000, *rb, dev)
    return torch.sort(a).values, torch.sort(b).values


def _unpaired(x, y):
    """mask of the elements of sorted x without a partner in sorted y, with existing ops (bar (a))"""
    lower = ops.searchsorted(y, x, values_sorted=True)
    upper = ops.searchsorted(y, x, right=True, values_sorted=True)
    return ops.run_positions(x) >= upper - lower


def _composition(x, y, op):
    """bar (a): (keys buffer, count) of the multiset op in keys mode"""
    if op == "intersection":
        return ops.compact(x, ~_unpaired(x, y))
    if op == "difference":
        return ops.compact(x, _unpaired(x, y))
    # the kept part of each side at exact size (one sync each, as a caller pays for it), then their merge
    right = ops.select(y, _unpaired(y, x))
    left = x if op == "union" else ops.select(x, _unpaired(x, y))
    out = ops.merge_keys(left, right)
    return out, torch.tensor(out.numel(), device=x.device)


def _torch_route(x, y, op):
    """bar (b), for duplicate-free sorted x and y"""
    if op == "intersection":
        return x[torch.isin(x, y, assume_unique=True)]
    if op == "difference":
        return x[~torch.isin(x, y, assume_unique=True)]
    return torch.unique(torch.cat([x, y]))


def _fmt(t):
    return f"{t[0]:.3f} / {t[1]:.3f}" if t else "n/a"


def _ratio(bar, ours):
    if not bar:
        return "n/a"
    r = f"{min(bar) / min(ours):.2f}x"
    return f"**{r} (slower)**" if min(ours) > min(bar) else r


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scale", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    half = (1 << 27) >> a.scale
    n = 2 * half
    src = torch.empty(2 * n + 4096, device=dev)  # copy floor buffers: up to 16 bytes per key moved
    dst = torch.empty_like(src)
    lines = [f"setops_lab: {half} + {half} keys, two runs of {a.reps} interleaved reps after {a.warmup} warm-ups, "
             f"{torch.cuda.get_device_name(0)}; ms are the medians of run 1 / run 2; ratios use the better run of each",
             "",
             "| op | mode | dtype | dist | kept | ours ms | (a) composition ms | (a) / ours | (b) torch ms | (b) / ours | "
             "(c) merge ms | ours / (c) | (d) copy_ ms | ours / (d) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    print("\n".join(lines), flush=True)
    rows = [(op, "keys", dt, "interleaved") for dt in ("f32", "i32") for op in OPS]
    if a.quick:
        rows += [("intersection", m, "f32", "interleaved") for m in ("index", "pairs")]
        rows += [("symmetric_difference", "keys", "f32", d) for d in ("disjoint", "identical", "ties", "equal")]
    else:
        rows += [(op, m, dt, "interleaved") for m in ("index", "pairs") for dt in ("f32", "i32") for op in OPS]
        rows += [(op, "keys", "f32", d) for d in ("disjoint", "identical", "ties", "equal") for op in OPS]
    ok = True
    for op, mode, dtype, dist in rows:
        x, y = _pair(half, dtype, dist, dev)
        vx = torch.arange(half, device=dev, dtype=torch.int32)
        vy = torch.arange(half, n, device=dev, dtype=torch.int32)
        if mode == "pairs":
            ours = lambda: ops.set_compact_by_key(x, vx, y, vy, op)  # noqa: E731
            merge = lambda: ops.merge_by_key(x, vx, y, vy)  # noqa: E731
        else:
            ours = lambda: ops.set_compact(x, y, op, indices=mode == "index")  # noqa: E731
            merge = (lambda: ops.merge(x, y)) if mode == "index" else (lambda: ops.merge_keys(x, y))  # noqa: E731
        got = ours()
        kept = int(got[-1])
        # the check: bar (a)'s formulation with torch ops, in merge order
        ux, uy = _unpaired_ref(x, y), _unpaired_ref(y, x)
        keep = {"intersection": (~ux, torch.zeros_like(uy)), "union": (torch.ones_like(ux), uy),
                "difference": (ux, torch.zeros_like(uy)), "symmetric_difference": (ux, uy)}[op]
        order = torch.sort(torch.cat([x, y]), stable=True).indices
        ref = order[torch.cat(keep)[order]]
        del ux, uy, keep, order
        same = kept == ref.numel() and torch.equal(got[0][:kept].view(torch.int32), torch.cat([x, y]).view(torch.int32)[ref])
        if mode != "keys":
            same = same and torch.equal(got[1][:kept], ref.int())
        del got, ref
        ok = ok and same
        fns = {"ours": ours}
        if mode == "keys":
            fns["comp"] = lambda: _composition(x, y, op)
        if (dtype, dist) == ("i32", "interleaved") and mode == "keys" and op != "symmetric_difference":
            if bool((x[1:] != x[:-1]).all()) and bool((y[1:] != y[:-1]).all()):
                fns["torch"] = lambda: _torch_route(x, y, op)
            else:  # full-range int32 draws collide now and then: bar (b) wants duplicate-free sides
                ux1, uy1 = torch.unique_consecutive(x), torch.unique_consecutive(y)
                fns["torch"] = lambda: _torch_route(ux1, uy1, op)
        fns["merge"] = merge
        m = (n * (8 if mode == "pairs" else 4) + kept * (4 if mode == "keys" else 8)) // 8
        fns["floor"] = lambda: ops.copy_(dst[:m], src[:m])
        t = _time_runs(fns, a.reps, a.warmup)
        lines.append(f"| {op} | {mode} | {dtype} | {dist} | {kept} | {_fmt(t['ours'])} | {_fmt(t.get('comp'))} | "
                     f"{_ratio(t.get('comp'), t['ours'])} | {_fmt(t.get('torch'))} | {_ratio(t.get('torch'), t['ours'])} | "
                     f"{_fmt(t['merge'])} | {min(t['ours']) / min(t['merge']):.2f}x | {_fmt(t['floor'])} | "
                     f"{min(t['ours']) / min(t['floor']):.2f}x |" + ("" if same else " MISMATCH"))
        print(lines[-1], flush=True)
        del x, y, vx, vy, fns
    lines += ["", f"outputs match the oracle: {ok}"]
    print(lines[-1])
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")
    return 0 if ok else 1


def _unpaired_ref(x, y):
    """_unpaired with torch ops only (the generated keys hold no NaN and no -0.0)"""
    i = torch.arange(x.numel(), device=x.device)
    rank = i - torch.searchsorted(x, x)
    return rank >= torch.searchsorted(y, x, right=True) - torch.searchsorted(y, x)


if __name__ == "__main__":
    raise SystemExit(main())
