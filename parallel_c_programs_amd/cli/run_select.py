"""Stream compaction CLI: keep the selected elements of N f32 per GPU in order, count them on the device (GB/s).

    run_select [N] [--keep F] [--mode mask|index|where] [--steps S --warmup W] [--no-check]

mask: values under a byte mask of keep fraction F; index: the int32 indices of the mask's nonzero elements (a
flattened nonzero); where: the values with x < F, no mask materialised. Prints the kept count, the reference's
"Time : %f s" line, the effective GB/s, and one JSON line (the check: every output and the count against torch, bit
for bit); exits 1 on a failed check. Ancestor: the pixel-stack frontier of ref 2-mpi-region-growing/region.c:493-533."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="f32 elements per GPU")
    ap.add_argument("--keep", type=float, default=0.5, help="fraction of the elements kept")
    ap.add_argument("--mode", choices=["mask", "index", "where"], default="mask")


def _report(out: dict) -> None:
    print(f"count : {out.get('kept', 'unchecked')}")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("select", argv, {"n": 1 << 28}, _args, lambda a: {"n": int(a.n), "keep": a.keep, "mode": a.mode},
              prog="run_select", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
