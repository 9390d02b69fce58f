"""Reduce / scan along a dimension CLI: op along the middle extent of an OUTER x N x INNER tensor per GPU.

    run_axis [OUTER] [N] [INNER] [--mode reduce|scan] [--op sum|min|max] [--dtype f32|i32] [--exclusive]
             [--route group|block|split|column|column_split] [--chunk C] [--steps S --warmup W] [--no-check]

INNER = 1 (the default) is the last-dimension case; INNER > 1 works down the columns of a row-major matrix. Prints the
element rate, the reference-style "Time : %f s" line, the effective GB/s of the work model (the input read once plus
what is written), and one JSON line (the check: every output against the host path of the same op on a host copy);
exits 1 on a failed check. No counterpart in the reference programs."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("outer", nargs="?", type=float, default=float(1 << 14), help="rows per GPU (slices when INNER > 1)")
    ap.add_argument("n", nargs="?", type=float, default=4096.0, help="elements along the dimension")
    ap.add_argument("inner", nargs="?", type=float, default=1.0, help="extent after the dimension (1: the last dim)")
    ap.add_argument("--mode", choices=["reduce", "scan"], default="reduce")
    ap.add_argument("--op", choices=["sum", "min", "max"], default="sum")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")
    ap.add_argument("--exclusive", action="store_true", help="scan: the exclusive form")
    ap.add_argument("--route", choices=["group", "block", "split", "column", "column_split"], default=None)
    ap.add_argument("--chunk", type=float, default=None, help="split routes: elements along N per chunk")


def _report(out: dict) -> None:
    print(f"{out['gelems_per_s']:.3f} Gelements/s")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("axis", argv, {"outer": 1 << 14, "n": 4096, "inner": 1},
              _args, lambda a: {"outer": int(a.outer), "n": int(a.n), "inner": int(a.inner), "mode": a.mode, "op": a.op,
                                "dtype": a.dtype, "exclusive": a.exclusive, "route": a.route,
                                "chunk": None if a.chunk is None else int(a.chunk)},
              prog="run_axis", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
