"""Radix sort CLI: stable sort of N keys per GPU (keys, key-value pairs or argsort), checked against torch.sort.

    run_sort [N] [--mode keys|pairs|argsort] [--dtype f32|i32] [--bits B] [--descending] [--steps S --warmup W] [--no-check]

keys: the sorted keys; pairs: the keys with an int32 payload; argsort: the int32 indices alone. --bits B (i32 only)
draws the keys from [0, 2^B) and sorts by the low B bits, ceil(B / 8) passes. Prints the pass count and key rate, the
reference-style "Time : %f s" line, the effective GB/s of the work model (histogram read + 4 bytes per key, and per
value, each way per pass), and one JSON line (the check: every output against torch.sort(stable=True), exactly); exits
1 on a failed check. No counterpart in the reference programs."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="keys per GPU")
    ap.add_argument("--mode", choices=["keys", "pairs", "argsort"], default="keys")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")
    ap.add_argument("--bits", type=int, default=None, help="i32 only: keys below 2^B, sorted by their low B bits")
    ap.add_argument("--descending", action="store_true")


def _report(out: dict) -> None:
    print(f"passes : {out['passes']}  {out['gkeys_per_s']:.3f} Gkeys/s")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("sort", argv, {"n": 1 << 28},
              _args, lambda a: {"n": int(a.n), "mode": a.mode, "dtype": a.dtype, "bits": a.bits,
                                "descending": a.descending},
              prog="run_sort", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
