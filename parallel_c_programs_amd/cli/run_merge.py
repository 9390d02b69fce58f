"""Merge / sorted-search CLI: N sorted keys per GPU in all, merged or searched (GB/s of the bytes a pass must move).

    run_merge [N] [--mode keys|pairs|index|search|search_sorted] [--dtype f32|i32] [--dist interleaved|disjoint|equal]
              [--split F] [--descending] [--right] [--steps S --warmup W] [--no-check]

keys / pairs / index: two sorted arrays of F * N and (1 - F) * N keys are merged (ops.merge_keys, ops.merge_by_key with
an int32 payload, ops.merge with int32 indices into the concatenation). search / search_sorted: F * N needles (in random
order / sorted, values_sorted=True) are looked up in a sorted haystack of (1 - F) * N keys (ops.searchsorted). dist
disjoint puts every key of a below every key of b; equal makes every comparison a tie. Prints the number of elements
checked, the reference's "Time : %f s" line, the effective GB/s, and one JSON line (the check: the output against the
stable torch.sort of the concatenation, or torch.searchsorted, exactly); exits 1 on a failed check."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="keys per GPU, both sides together")
    ap.add_argument("--mode", choices=["keys", "pairs", "index", "search", "search_sorted"], default="keys")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")
    ap.add_argument("--dist", choices=["interleaved", "disjoint", "equal"], default="interleaved")
    ap.add_argument("--split", type=float, default=0.5, help="fraction of N that is a (merge) or the needles (search)")
    ap.add_argument("--descending", action="store_true")
    ap.add_argument("--right", action="store_true", help="search: upper instead of lower bound")


def _report(out: dict) -> None:
    print(f"elements checked : {out.get('elements_checked', 'unchecked')}")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("merge", argv, {"n": 1 << 28}, _args,
              lambda a: {"n": int(a.n), "mode": a.mode, "dtype": a.dtype, "dist": a.dist, "split": a.split,
                         "descending": a.descending, "right": a.right},
              prog="run_merge", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
