"""Ragged segment sort CLI: the keys of every segment that an offsets tensor cuts out of N keys per GPU, sorted on
their own.

    run_segsort [N] [--mean-len L] [--dist uniform|equal|powerlaw|empty] [--mode keys|index|pairs] [--dtype f32|i32]
                [--descending] [--route classes|global] [--max-len M] [--steps S --warmup W] [--no-check]

Prints the key rate, the reference-style "Time : %f s" line, the effective GB/s of the work model (the keys and the
offsets read once, every output written once), and one JSON line (the check: every output against the host path on a
host copy, bit for bit); exits 1 on a failed check. No counterpart in the reference programs."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n", nargs="?", type=float, default=float(1 << 28), help="keys per GPU")
    ap.add_argument("--mean-len", type=float, default=100.0, help="mean segment length (N for one segment)")
    ap.add_argument("--dist", choices=["uniform", "equal", "powerlaw", "empty"], default="uniform")
    ap.add_argument("--mode", choices=["keys", "index", "pairs"], default="keys")
    ap.add_argument("--dtype", choices=["f32", "i32"], default="f32")
    ap.add_argument("--descending", action="store_true")
    ap.add_argument("--route", choices=["classes", "global"], default=None, help="force a route (default: by length)")
    ap.add_argument("--max-len", type=int, default=None, help="a promised bound on the segment length")


def _report(out: dict) -> None:
    print(f"{out['gkeys_per_s']:.3f} Gkeys/s")
    print(f"{out['value']:.1f} {out['unit']}")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("segsort", argv, {"n": 1 << 28},
              _args, lambda a: {"n": int(a.n), "mean_len": a.mean_len, "dist": a.dist, "mode": a.mode, "dtype": a.dtype,
                                "descending": a.descending, "route": a.route, "max_len": a.max_len},
              prog="run_segsort", doc=__doc__, time_line=True)
    if out is not None:
        _report(out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
