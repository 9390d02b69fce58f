"""Scan-by-key CLI: the running sum, min or max inside every run of equal neighbouring keys of N elements per GPU (GB/s).

    run_scanbykey [N] [--mean-run R] [--op sum|min|max] [--dtype f32|i32] [--exclusive] [--mode keys|heads|positions]
                  [--steps S --warmup W] [--no-check]

keys: int32 keys, values of the given dtype scanned per run (ops.scan_by_key); heads: the same runs given as bool head
flags (ops.segmented_scan); positions: the index of every element inside its run (ops.run_positions, no values). Run
lengths are geometric with mean R (0: every key equal, one run across the whole input). Prints the run count, the
reference's "Time : %f s" line, the effective GB/s, and one JSON line (the check: every output against an exact int64 /
fp64 oracle); exits 1 on a failed check."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="elements per GPU")
    ap.add_argument("--mean-run", type=float, default=4.0, help="mean run length (0: all keys equal)")
    ap.add_argument("--op", choices=["sum", "min", "max"], default="sum")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")
    ap.add_argument("--exclusive", action="store_true")
    ap.add_argument("--mode", choices=["keys", "heads", "positions"], default="keys")


def _report(out: dict) -> None:
    print(f"runs : {out.get('runs', 'unchecked')}")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("scanbykey", argv, {"n": 1 << 28}, _args,
              lambda a: {"n": int(a.n), "mean_run": a.mean_run, "op": a.op, "dtype": a.dtype, "exclusive": a.exclusive,
                         "mode": a.mode},
              prog="run_scanbykey", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
