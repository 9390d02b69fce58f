"""argmin / argmax CLI: where the extremum is, and its value, per GPU.

    run_argreduce [N] [--form flat|dim|segments] [--op max|min] [--dtype f32|i32]
                  [--outer O --inner I --route group|block|split|column|column_split --chunk C]   (form dim)
                  [--mean-len L --dist uniform|equal|powerlaw|empty]                              (form segments)
                  [--steps S --warmup W] [--no-check]

flat: one extremum of N elements. dim: along the middle extent of an OUTER x N x INNER tensor (INNER = 1 is the
last-dimension case). segments: one extremum per segment that an offsets tensor cuts out of N elements. Prints the
element rate, the reference-style "Time : %f s" line, the effective GB/s of the work model (the input read once, a
value and an index written per result), and one JSON line (the check: values as bit patterns and indices against the
host path on a host copy); exits 1 on a failed check. No counterpart in the reference programs."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="elements (form dim: along the dimension)")
    ap.add_argument("--form", choices=["flat", "dim", "segments"], default="flat")
    ap.add_argument("--op", choices=["max", "min"], default="max")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")
    ap.add_argument("--outer", type=float, default=float(1 << 14), help="form dim: rows (slices when INNER > 1)")
    ap.add_argument("--inner", type=float, default=1.0, help="form dim: extent after the dimension (1: the last dim)")
    ap.add_argument("--route", choices=["group", "block", "split", "column", "column_split"], default=None)
    ap.add_argument("--chunk", type=float, default=None, help="form dim, split routes: elements along N per chunk")
    ap.add_argument("--mean-len", type=float, default=100.0, help="form segments: mean segment length")
    ap.add_argument("--dist", choices=["uniform", "equal", "powerlaw", "empty"], default="uniform")


def _report(out: dict) -> None:
    print(f"{out['gelems_per_s']:.3f} Gelements/s")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("argreduce", argv, {"n": 1 << 28},
              _args, lambda a: {"n": int(a.n), "form": a.form, "op": a.op, "dtype": a.dtype, "outer": int(a.outer),
                                "inner": int(a.inner), "route": a.route, "chunk": None if a.chunk is None else int(a.chunk),
                                "mean_len": a.mean_len, "dist": a.dist},
              prog="run_argreduce", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
