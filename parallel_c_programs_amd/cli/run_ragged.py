"""Ragged segment reduction CLI: op over the segments that an offsets tensor cuts out of N elements per GPU.

    run_ragged [N] [--mean-len L] [--dist uniform|equal|powerlaw|empty] [--op sum|min|max] [--dtype f32|i32]
               [--steps S --warmup W] [--no-check]

Prints the element rate, the reference-style "Time : %f s" line, the effective GB/s of the work model (the elements and
the offsets read once, one result per segment written), and one JSON line (the check: every result against the host
path on a host copy); exits 1 on a failed check. No counterpart in the reference programs."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="elements per GPU")
    ap.add_argument("--mean-len", type=float, default=100.0, help="mean segment length (N for one segment)")
    ap.add_argument("--dist", choices=["uniform", "equal", "powerlaw", "empty"], default="uniform")
    ap.add_argument("--op", choices=["sum", "min", "max"], default="sum")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")


def _report(out: dict) -> None:
    print(f"{out['gelems_per_s']:.3f} Gelements/s")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("ragged", argv, {"n": 1 << 28},
              _args, lambda a: {"n": int(a.n), "mean_len": a.mean_len, "dist": a.dist, "op": a.op, "dtype": a.dtype},
              prog="run_ragged", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
