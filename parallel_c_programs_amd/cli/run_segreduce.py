"""Run-length encode / reduce-by-key CLI: collapse the runs of equal neighbouring keys of N elements per GPU (GB/s).

    run_segreduce [N] [--mean-run R] [--mode rle|sum|unique] [--dtype f32|i32] [--steps S --warmup W] [--no-check]

rle: run keys and lengths of keys of the given dtype; sum: int32 keys, values of the given dtype summed per run;
unique: sorted distinct values and counts of an unsorted input (sort, then collapse). Run lengths are geometric with
mean R (0: every key equal, one run across the whole input). Prints the run count, the reference's "Time : %f s" line,
the effective GB/s, and one JSON line (the check: every output against torch); exits 1 on a failed check."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="elements per GPU")
    ap.add_argument("--mean-run", type=float, default=4.0, help="mean run length (0: all keys equal)")
    ap.add_argument("--mode", choices=["rle", "sum", "unique"], default="rle")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")


def _report(out: dict) -> None:
    print(f"runs : {out.get('runs', 'unchecked')}")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("segreduce", argv, {"n": 1 << 28},
              _args, lambda a: {"n": int(a.n), "mean_run": a.mean_run, "mode": a.mode, "dtype": a.dtype},
              prog="run_segreduce", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
