"""SpMM CLI: a CSR matrix times a dense block of K vectors per GPU (ops.spmm, csrc/kernels/spmm.hip).

    run_spmm [N_ROWS] [NNZ] [--k K] [--matrix powerlaw|banded|uniform] [--item-nnz I] [--steps S --warmup W] [--no-check]

powerlaw: the synthetic power-law graph of run_workload spmv; banded: the reference's 5-band geometry (401 200 100 200
10) on N_ROWS rows (NNZ follows from it); uniform: every row NNZ / N_ROWS nonzeros in uniformly drawn columns. --item-nnz:
the plan's item size, a multiple of 64 in 64..1024 (default: by K). Prints GFLOP/s (2 NNZ K / time), the compulsory
traffic (col and val, X and Y once) and the gathered bytes (4 K NNZ) per second, the reference-style "Time : %f s" line
and one JSON line; the check compares a fixed seeded sample of rows with the fp64 product inside the any-order rounding
bound and prints `checks_passed`; a failed check exits 1. No counterpart in the reference programs."""
import sys

from .run_workload import run


def _args(ap):
    ap.add_argument("n_rows", nargs="?", type=float, default=1e6, help="rows (and columns) of the matrix")
    ap.add_argument("nnz", nargs="?", type=float, default=1e7, help="nonzeros (powerlaw: the target; banded: ignored)")
    ap.add_argument("--k", type=int, default=64, help="columns of the dense block")
    ap.add_argument("--matrix", choices=["powerlaw", "banded", "uniform"], default="powerlaw")
    ap.add_argument("--item-nnz", type=int, default=None, help="nonzeros per work item (multiple of 64 in 64..1024)")


def main(argv=None) -> int:
    argv = sys.argv[1:] if argv is None else list(argv)
    out = run("spmm", argv, {}, _args,
              lambda a: {"n_rows": int(a.n_rows), "nnz": int(a.nnz), "k": a.k, "matrix": a.matrix, "item_nnz": a.item_nnz},
              prog="run_spmm", doc=__doc__, time_line=True)
    if out is not None:
        print(f"{out['value']:.1f} {out['unit']}, {out['compulsory_gb_per_s']:.1f} GB/s compulsory, "
              f"{out['gathered_gb_per_s']:.1f} GB/s gathered")
        if out.get("check_passed"):
            print(f"checks_passed ({out['rows_checked']} rows against fp64, worst error / bound "
                  f"{out['worst_err_over_bound']:.3f})")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
