"""Set-operation CLI: N sorted keys per GPU in all, split into two sorted arrays, combined by one set operation (GB/s
of the bytes the pass moves: both inputs read once, every kept element written once).

    run_setops [N] [--op intersection|union|difference|symmetric_difference] [--mode keys|index|pairs]
               [--dtype f32|i32] [--dist interleaved|disjoint|identical|ties|equal] [--split F] [--descending]
               [--steps S --warmup W] [--no-check]

Two sorted arrays of F * N and (1 - F) * N keys go through ops.set_compact (keys), ops.set_compact with int32 indices
into the concatenation (index) or ops.set_compact_by_key with an int32 payload (pairs); the timed step does not
synchronise. dist disjoint puts every key of a below every key of b, identical makes both sides prefixes of one sorted
array, ties draws from eight keys, equal makes every comparison a tie. Prints the number of elements checked and
kept, the reference's "Time : %f s" line, the effective GB/s, and one JSON line (the check: count, keys, and indices
or payload against the runs of the stable torch.sort of the concatenation, exactly); exits 1 on a failed check."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="keys per GPU, both sides together")
    ap.add_argument("--op", choices=["intersection", "union", "difference", "symmetric_difference"], default="intersection")
    ap.add_argument("--mode", choices=["keys", "index", "pairs"], default="keys")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")
    ap.add_argument("--dist", choices=["interleaved", "disjoint", "identical", "ties", "equal"], default="interleaved")
    ap.add_argument("--split", type=float, default=0.5, help="fraction of N that is a")
    ap.add_argument("--descending", action="store_true")


def _report(out: dict) -> None:
    print(f"elements checked : {out.get('elements_checked', 'unchecked')}")
    print(f"elements kept : {out['kept']}")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("setops", argv, {"n": 1 << 28}, _args,
              lambda a: {"n": int(a.n), "op": a.op, "mode": a.mode, "dtype": a.dtype, "dist": a.dist, "split": a.split,
                         "descending": a.descending},
              prog="run_setops", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
