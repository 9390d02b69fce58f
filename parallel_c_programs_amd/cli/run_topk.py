"""Top-k CLI: the K best of N keys per GPU and their indices by radix select, checked against torch.sort.

    run_topk [N] [--k K] [--smallest] [--unsorted] [--dtype f32|i32] [--dist uniform|equal|sorted] [--method select|sort]
             [--steps S --warmup W] [--no-check]

The K largest (--smallest: smallest) keys with their int32 indices, in sorted order (--unsorted: in index order). Prints
the key rate, the reference-style "Time : %f s" line, the effective GB/s of the work model (five reads of the keys plus
the survivors' gather and sort), and one JSON line (the check: values and indices against the first K entries of
torch.sort(stable=True), exactly); exits 1 on a failed check. No counterpart in the reference programs."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="keys per GPU")
    ap.add_argument("--k", type=float, default=1024.0, help="how many of the best keys")
    ap.add_argument("--smallest", action="store_true")
    ap.add_argument("--unsorted", action="store_true")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")
    ap.add_argument("--dist", choices=["uniform", "equal", "sorted"], default="uniform")
    ap.add_argument("--method", choices=["select", "sort"], default=None)


def _report(out: dict) -> None:
    print(f"k : {out['k']}  {out['gkeys_per_s']:.3f} Gkeys/s")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("topk", argv, {"n": 1 << 28},
              _args, lambda a: {"n": int(a.n), "k": int(a.k), "dtype": a.dtype, "largest": not a.smallest,
                                "sorted": not a.unsorted, "dist": a.dist, "method": a.method},
              prog="run_topk", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
