"""Histogram CLI: int32 counts of N samples per GPU in B bins (GB/s of samples read).

    run_bincount [N] [--bins B] [--dist uniform|equal|sorted|zipf] [--dtype i32|u8|f32] [--mode bincount|histc|edges]
                 [--weights none|i32|f32] [--steps S --warmup W] [--no-check]

bincount: the value of an i32 / u8 sample is its bin (ops.bincount; int32 weights are summed in the same kernel, float32
weights take the sort route); histc: f32 samples in B equal-width bins of [0, 1] (ops.histc); edges: the same bins given
as B + 1 explicit edges (ops.histogram, at most 8192 bins). dist equal puts every sample in one bin. Prints the number
of samples counted, the reference's "Time : %f s" line, the effective GB/s, and one JSON line (the check: the counts
against torch.bincount of the oracle bins, exactly); exits 1 on a failed check. cli/run_histogram.py is the reference's
program 4 (histogram equalisation of an image) and is a different tool."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="samples per GPU")
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--dist", choices=["uniform", "equal", "sorted", "zipf"], default="uniform")
    ap.add_argument("--dtype", choices=["i32", "u8", "f32"], default=None, help="default: i32, f32 for histc / edges")
    ap.add_argument("--mode", choices=["bincount", "histc", "edges"], default="bincount")
    ap.add_argument("--weights", choices=["none", "i32", "f32"], default="none")


def _report(out: dict) -> None:
    print(f"samples counted : {out.get('samples_counted', 'unchecked')}")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("bincount", argv, {"n": 1 << 28}, _args,
              lambda a: {"n": int(a.n), "num_bins": a.bins, "dist": a.dist,
                         "dtype": a.dtype or ("i32" if a.mode == "bincount" else "f32"), "mode": a.mode,
                         "weights": a.weights},
              prog="run_bincount", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
