"""Row-wise sort CLI: every row of a ROWS x COLS matrix per GPU sorted, or its top-k / k-th value, along the last dim.

    run_rowsort [ROWS] [COLS] [--mode keys|index|pairs|topk|kth] [--k K] [--dtype f32|i32] [--descending]
                [--route wave|block|loop|global|sortkeep|select] [--steps S --warmup W] [--no-check]

Prints the key rate, the reference-style "Time : %f s" line, the effective GB/s of the work model (the keys read once
plus what is written), and one JSON line (the check: every output against torch.sort(dim=-1, stable=True) of a host
copy, exactly); exits 1 on a failed check. No counterpart in the reference programs."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("rows", nargs="?", type=float, default=float(1 << 14), help="rows per GPU")
    ap.add_argument("cols", nargs="?", type=float, default=4096.0, help="keys per row")
    ap.add_argument("--mode", choices=["keys", "index", "pairs", "topk", "kth"], default="keys")
    ap.add_argument("--k", type=float, default=64.0, help="topk / kth: how many of the best keys, or which")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")
    ap.add_argument("--descending", action="store_true", help="topk / kth: the largest")
    ap.add_argument("--route", choices=["wave", "block", "loop", "global", "sortkeep", "select"], default=None)


def _report(out: dict) -> None:
    print(f"{out['gkeys_per_s']:.3f} Gkeys/s")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("rowsort", argv, {"rows": 1 << 14, "cols": 4096},
              _args, lambda a: {"rows": int(a.rows), "cols": int(a.cols), "mode": a.mode, "k": int(a.k), "dtype": a.dtype,
                                "descending": a.descending, "route": a.route},
              prog="run_rowsort", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
