"""Step-able workloads with work models. Every workload owns its per-rank data (weak scaling unless noted),
exposes step() (one timed unit of work, including its collectives) and report(seconds, steps) (whole-job
throughput = sum over ranks), and check() (a numerics check against an independent reference)."""
from __future__ import annotations

import os
from dataclasses import dataclass, field

import torch

from .. import ops
from ..ops.sparse import powerlaw_row_ptr
from ..ops.vector import SET_OP_CODES, _axis_plan
from ..parallel.collectives import global_scan
from ..parallel.dist import Context

# Pass threshold of every fp64-referenced numerics check (relative error): bench.py fails the run above it, and
# run_workload exits 1. Bit-exact checks (stencil, region growing, histogram) pass only when exact.
REL_ERR_LIMIT = 1e-5


@dataclass
class Workload:
    ctx: Context
    cfg: dict = field(default_factory=dict)
    name: str = ""
    unit: str = ""

    def step(self) -> None:  # pragma: no cover - interface
        raise NotImplementedError

    def work_per_step(self) -> float:
        """Units of work per step per rank (flops, bytes, updates...)."""
        raise NotImplementedError

    def scale(self) -> float:
        return 1e12 if self.unit == "TFLOPS" else 1e9

    def report(self, seconds: float, steps: int) -> dict:
        total = self.ctx.world * self.work_per_step() * steps / seconds / self.scale()
        return {"value": total, "unit": self.unit, "ms_per_step": 1e3 * seconds / steps}

    def check(self, reduce: bool = True) -> dict:
        """Numerics check against an independent reference: a dict with "check_passed" (bool) and the measured
        error(s). reduce=False returns THIS rank's values without the final reduction over ranks (bench.py merges
        them in its own collective decision step); every collective a check needs runs before its local-only part,
        so a local failure cannot leave another rank waiting in a data collective."""
        return {"check_passed": True}

    def compute_only_step(self) -> None:
        """The same kernels on the same data as step(), with every inter-rank exchange skipped (N > 1 attribution:
        full step minus this = the exposed communication; ref 2-mpi-region-growing/region.c:497-532 separates the
        exchange from the compute the same way). Leaves the workload's state unchecked: run it after check()."""
        self.step()

    def bytes_exchanged_per_step(self) -> float:
        """Payload bytes this rank SENDS to other ranks per step (averaged over a deep-halo period)."""
        return 0.0


class Sgemm(Workload):
    """C = A @ B, fp32 exact (MFMA v_mfma_f32_32x32x2_f32), per-rank operands (data-parallel, weak)."""

    def __init__(self, ctx, n=8192, variant=-1, **_):
        super().__init__(ctx, {"n": n, "variant": variant}, "sgemm", "TFLOPS")
        dev = ctx.device
        self.a = torch.empty(n, n, device=dev)
        self.b = torch.empty(n, n, device=dev)
        self.c = torch.empty(n, n, device=dev)
        ops.rand_uniform_(self.a, 1000 + ctx.rank)
        ops.rand_uniform_(self.b, 2000 + ctx.rank)
        self.n, self.variant = n, variant

    def step(self):
        if self.ctx.device.type == "cuda":
            ops.sgemm_out(self.a, self.b, self.c, variant=self.variant)
        else:
            torch.matmul(self.a, self.b, out=self.c)

    def work_per_step(self):
        return 2.0 * self.n ** 3

    def check(self, reduce: bool = True, block_rows: int = 2048):
        """EVERY element of the timed C against an fp64 GEMM of the same operands (row blocks of block_rows, so the
        fp64 copy of A is never whole), relative to max |C_ref| (ref 3-serial-optimization/spmv.c:179-191 compares
        every output too). Local only."""
        bd = self.b.double()
        err = torch.zeros((), dtype=torch.float64, device=self.a.device)
        big = torch.zeros((), dtype=torch.float64, device=self.a.device)
        for s in range(0, self.n, block_rows):
            ref = self.a[s:s + block_rows].double() @ bd
            err = torch.maximum(err, (self.c[s:s + block_rows].double() - ref).abs().max())
            big = torch.maximum(big, ref.abs().max())
            del ref
        del bd
        e = (err / big.clamp_min(1e-300)).item()
        if reduce:
            e = self.ctx.max_over_ranks(e)
        return {"max_rel_err_vs_fp64": e, "elements_checked": self.n * self.n, "check_passed": e <= REL_ERR_LIMIT}


class Reduce(Workload):
    """Global sum of world x n f32: local HBM-bound reduction + one-scalar RCCL all-reduce.

    With several ranks a step's all-reduce is left in flight on RCCL's stream and overlaps the NEXT step's local
    reduction: step k launches its reduction, then makes the compute stream wait for step k-1's all-reduce and stores
    that global total, then posts its own all-reduce. Every all-reduce is enqueued inside the step that computed its
    input and completes on the device before the bench's closing synchronize; settle() (called by check()) stores the
    last one's total."""

    def __init__(self, ctx, n=10**9, **_):
        super().__init__(ctx, {"n": n}, "reduce", "GB/s")
        self.x = torch.empty(int(n), device=ctx.device)
        ops.rand_uniform_(self.x, 3000 + ctx.rank, 0.0, 1.0)
        self.total = torch.zeros((), device=ctx.device)
        self._pending = None  # (work, partial sum) of the all-reduce still in flight
        self.overlap = os.environ.get("PCMX_REDUCE_OVERLAP", "1") != "0"  # 0: the round-5 blocking all-reduce

    def step(self):
        s = ops.reduce(self.x, "sum").reshape(1).float()
        if not self.ctx.distributed or not self.overlap:
            self.ctx.all_reduce_(s)
            self.total.copy_(s.reshape(()))
            return
        self.settle()
        self._pending = (self.ctx.all_reduce_async(s), s)

    def settle(self):
        """The compute stream waits for the all-reduce in flight (if any) and stores its global total."""
        if self._pending is not None:
            work, s = self._pending
            self._pending = None
            work.wait()
            self.total.copy_(s.reshape(()))

    def compute_only_step(self):
        self.settle()
        self.total.copy_(ops.reduce(self.x, "sum").reshape(()).float())

    def bytes_exchanged_per_step(self):
        return 4.0 if self.ctx.distributed else 0.0  # one f32 into the all-reduce

    def work_per_step(self):
        return 4.0 * self.x.numel()

    def check(self, reduce: bool = True):
        self.settle()
        ref = self.x.double().sum().reshape(1)
        self.ctx.all_reduce_(ref)  # (the one collective, before the local comparison)
        e = abs(self.total.item() - ref.item()) / max(abs(ref.item()), 1e-300)
        if reduce:
            e = self.ctx.max_over_ranks(e)
        return {"rel_err_vs_fp64": e, "check_passed": e <= REL_ERR_LIMIT}


class Axpy(Workload):
    """y <- alpha x + y over n f32 per GPU (the north star's AXPY hot loop; ref 6-opencl-region-growing/
    multiply_opencl.cl:1-4 is its element-wise ancestor): 12 B/element of HBM traffic per step, weak scaling, no
    communication. The ticket-ordered streaming kernel (csrc/kernels/vector.hip).

    The data make every step EXACT in fp32, so the timed output itself is checkable bit for bit after any number of
    steps: x = k / 2^11 (k < 2^11), y0 on the 2^-23 grid in [0, 1), alpha = 2^-12; every increment alpha x is then a
    multiple of 2^-23 and y stays below 2 (where that grid is representable) for fewer than 4096 steps."""

    ALPHA = 2.0 ** -12

    def __init__(self, ctx, n=10**9, **_):
        super().__init__(ctx, {"n": n, "alpha": self.ALPHA}, "axpy", "GB/s")
        self.x = torch.empty(int(n), device=ctx.device)
        self.y = torch.empty(int(n), device=ctx.device)
        ops.rand_uniform_(self.x, 5000 + ctx.rank, 0.0, 1.0)
        ops.rand_uniform_(self.y, 6000 + ctx.rank, 0.0, 1.0)
        self.x.mul_(2048.0).floor_().div_(2048.0)
        self.y.mul_(2.0 ** 23).floor_().div_(2.0 ** 23)
        self.y0 = self.y.clone()
        self.alpha, self.steps = self.ALPHA, 0

    def step(self):
        ops.axpy_(self.y, self.alpha, self.x)
        self.steps += 1

    def torch_step(self):
        """The same update through torch (the vendor bar); counted like a step."""
        self.y.add_(self.x, alpha=self.alpha)
        self.steps += 1

    def work_per_step(self):
        return 12.0 * self.x.numel()

    def check(self, reduce: bool = True, chunk: int = 1 << 26):
        """EVERY element of the timed output against fp64 y0 + steps * alpha * x (exact while steps < 4096), relative
        to max |y|. Local only."""
        err = torch.zeros((), dtype=torch.float64, device=self.x.device)
        big = torch.zeros((), dtype=torch.float64, device=self.x.device)
        n, a = self.x.numel(), self.steps * self.alpha
        for s0 in range(0, n, chunk):
            ref = self.y0[s0:s0 + chunk].double() + a * self.x[s0:s0 + chunk].double()
            err = torch.maximum(err, (self.y[s0:s0 + chunk].double() - ref).abs().max())
            big = torch.maximum(big, ref.abs().max())
        e = (err / big.clamp_min(1e-300)).item()
        if reduce:
            e = self.ctx.max_over_ranks(e)
        return {"rel_err_vs_fp64": e, "steps_applied": self.steps, "check_passed": e <= REL_ERR_LIMIT}


class Scan(Workload):
    """Inclusive prefix sum across ranks: local totals all-gathered, rank offset fed to the single-pass
    decoupled look-back scan as its initial value."""

    def __init__(self, ctx, n=10**9, **_):
        super().__init__(ctx, {"n": n}, "scan", "GB/s")
        self.x = torch.empty(int(n), device=ctx.device)
        ops.rand_uniform_(self.x, 4000 + ctx.rank, 0.0, 1.0)
        self.y = None

    def step(self):
        self.y = global_scan(self.x, self.ctx)

    def compute_only_step(self):
        self.y = global_scan(self.x, self.ctx, comm=False)

    def bytes_exchanged_per_step(self):
        return 4.0 if self.ctx.distributed else 0.0  # this rank's total into the all-gather

    def work_per_step(self):
        # effective bandwidth: the 8 B/element a scan must move (read + write); with several ranks the extra
        # 4 B/element reduce pass that seeds each rank's offset counts as time, not as work
        return 8.0 * self.x.numel()

    def check(self, reduce: bool = True, chunk: int = 1 << 26, one_rank_at_a_time: bool = False):
        """Every output of the timed scan (all n, not a prefix) against an fp64 cumsum carried across chunks, seeded
        with this rank's offset (the fp64 sum of the lower ranks' totals), and the look-back error word of the
        stream (lookback_ok False if any timed scan gave up a look-back). The totals' all-gather runs first: a rank
        whose stream reports a timed-out look-back still joins it, then reports the flag instead of raising.
        one_rank_at_a_time (ranks sharing one GPU): the ranks take turns for the fp64 cumsums, behind barriers.
        torch.cumsum is rocPRIM's look-back scan, which waits on blocks by index, and several processes' copies of it
        on one GPU can starve each other's predecessors."""
        tot = self.x.double().sum().reshape(1)
        totals = self.ctx.all_gather(tot)
        lookback_ok = True
        if self.x.is_cuda:
            try:
                ops.scan_check(self.x.device)
            except RuntimeError:
                lookback_ok = False
        carry = torch.zeros((), dtype=torch.float64, device=self.x.device)
        for t in totals[: self.ctx.rank]:
            carry = carry + t.to(carry.device).reshape(())
        err = torch.zeros((), dtype=torch.float64, device=self.x.device)
        n = self.x.numel()
        for turn in range(self.ctx.world if one_rank_at_a_time else 1):
            if one_rank_at_a_time and turn != self.ctx.rank:
                self.ctx.barrier()
                continue
            for s in range(0, n, chunk):
                ref = torch.cumsum(self.x[s:s + chunk].double(), 0) + carry
                err = torch.maximum(err, (self.y[s:s + chunk].double() - ref).abs().max())
                carry = ref[-1]
            if one_rank_at_a_time:
                if self.x.is_cuda:
                    torch.cuda.synchronize(self.x.device)
                self.ctx.barrier()
        # relative to this rank's largest prefix (its last one: the inputs are non-negative)
        e = (err / carry.abs().clamp_min(1e-30)).item()
        if reduce:
            e = self.ctx.max_over_ranks(e)
            lookback_ok = self.ctx.max_over_ranks(0.0 if lookback_ok else 1.0) == 0.0
        return {"rel_err_vs_fp64": e, "elements_checked": n, "lookback_ok": lookback_ok,
                "check_passed": e <= REL_ERR_LIMIT and lookback_ok}


class Stencil(Workload):
    """16384^2 bf16 5-point stencil, row slabs + halo exchange overlapped with the interior update.
    Strong scaling across ranks when `global_n` is fixed (the grid is split); weak when `per_rank`.
    fuse=T (default 0: auto_fuse of the slab height): T time steps per kernel (temporal blocking, bit-identical to single steps) and a T-row
    halo exchange every T steps; one step() then advances T time steps and counts T updates per cell."""

    def __init__(self, ctx, n=16384, per_rank=False, overlap=True, graph_steps=0, fuse=0, halo_mult=0,
                 pattern="random", **_):
        from ..parallel.stencil import StencilSlab, auto_fuse, auto_halo_mult

        rows = n * (ctx.world if per_rank else 1)
        fuse = int(fuse) or auto_fuse(rows // ctx.world)
        auto_m = not int(halo_mult)
        halo_mult = int(halo_mult) or auto_halo_mult(rows // ctx.world, fuse, ctx.world)
        self.ctx, self.overlap, self.pattern = ctx, overlap, pattern
        # The deep halo (m > 1) is proven on this job's own backend before it is timed: a small grid through the same
        # slab code at this world size must equal the single-domain oracle bit for bit; an AUTO depth that fails it
        # falls back to m = 1 (halo_selftest False in the line), an explicit one stays and fails the check.
        self.halo_selftest = None
        if halo_mult > 1 and ctx.distributed:
            self.halo_selftest = self._small_grid_ok(fuse, halo_mult)
            if not self.halo_selftest and auto_m:
                halo_mult = 1
        super().__init__(ctx, {"n": n, "rows": rows, "graph_steps": graph_steps, "fuse": fuse,
                               "halo_mult": halo_mult, "pattern": pattern}, "stencil", "GLUP/s")
        self.slab = StencilSlab(ctx, rows, n, fuse=fuse, halo_mult=halo_mult, pattern=pattern)
        self.graph_steps = graph_steps  # >0: one step() = graph_steps updates replayed from a HIP graph
        self.cells_local = self.slab.rows * n

    def step(self):
        if self.graph_steps:
            self.slab.run(self.graph_steps, self.overlap, graph=True)
        else:
            self.slab.step(self.overlap)

    def compute_only_step(self):
        self.slab.step(self.overlap, comm=False)

    def bytes_exchanged_per_step(self):
        return self.slab.halo_bytes_per_step()

    def work_per_step(self):
        return float(self.cells_local) * (self.graph_steps or self.slab.fuse)

    def report(self, seconds, steps):
        r = super().report(seconds, steps)
        # strong scaling (one fixed grid): the world-sum of local cells is the grid, not world x grid
        t = self.ctx.scalar(float(self.cells_local))
        self.ctx.all_reduce_(t)
        r["value"] = t.item() * (self.graph_steps or self.slab.fuse) * steps / seconds / 1e9
        return r

    def check(self, reduce: bool = True):
        """Two bit-exact checks.
        small grid: a small grid stepped through the same slab code at this world size (row slabs, fused T-row
          halo exchange, overlap) against the single-domain single-step oracle (collectives: it runs first);
        timed grid: the grid the timed steps produced (warm-up + timed, `steps_done` updates of the full 16384^2
          problem, this rank's rows) against a plain-PyTorch f32 single-step oracle of the whole grid
          (ops.stencil5_reference, bf16 rounding per step) run on this rank's device (local only)."""
        from ..parallel.stencil import reference_run_torch

        sl = self.slab
        ok = self._small_grid_ok(sl.fuse, sl.m)
        ref = reference_run_torch(sl.n, sl.steps_done, sl.cols, sl.k, device=self.ctx.device, pattern=self.pattern)
        mine = sl.interior()
        timed_ok = torch.equal(mine.view(torch.int16), ref[sl.row0:sl.row0 + sl.rows].view(torch.int16))
        del ref
        finite = bool(torch.isfinite(mine.float()).all())
        if reduce:
            timed_ok = self.ctx.max_over_ranks(0.0 if timed_ok else 1.0) == 0.0
            finite = self.ctx.max_over_ranks(0.0 if finite else 1.0) == 0.0
        return {"timed_grid_bit_exact": bool(timed_ok), "timed_grid_updates": sl.steps_done,
                "bit_exact_vs_single_step_oracle": bool(ok), "finite": bool(finite), "halo_selftest": self.halo_selftest,
                "check_passed": bool(timed_ok and ok and finite)}

    def _small_grid_ok(self, f: int, m: int) -> bool:
        """A small random grid stepped through the same slab code at this world size (row slabs, the fused / deep
        halo exchange, overlap) equals the single-domain single-step oracle bit for bit (collective; same answer on
        every rank)."""
        from ..parallel.stencil import StencilSlab, reference_run

        n, cols, steps = max(64, 2 * f * m * self.ctx.world + 8), 200, 4 * f * max(1, m)
        small = StencilSlab(self.ctx, n, cols, fuse=f, halo_mult=m, pattern=self.pattern)
        small.run(steps, self.overlap)
        full = small.gather()
        ok = 1.0
        if self.ctx.is_root:
            ref = reference_run(n, steps, cols, device=self.ctx.device, pattern=self.pattern)
            ok = float(torch.equal(full.view(torch.int16), ref.view(torch.int16)))
        return self.ctx.broadcast_(self.ctx.scalar(ok)).item() == 1.0


class SpMV(Workload):
    """Power-law CSR SpMV (nnz-balanced row blocks) + chunked exchange of y overlapped with the product
    (parallel/spmv.py): y <- A x in each rank's layout (own rows + ghosts by default, or the replicated padded
    layout with exchange="allgather"). Strong scaling: one fixed matrix."""

    def __init__(self, ctx, n_rows=10_000_000, nnz=100_000_000, alpha=2.5, slices=-1, head=0.0625,
                 balance=0.0, chunks=0, exchange="ghost", keep_plain=False, colsplit=None, **_):
        from ..parallel.spmv import DistributedSpMV

        slices = int(slices) if ctx.device.type == "cuda" else 0
        self.d = DistributedSpMV.powerlaw(ctx, n_rows, nnz, alpha, slices=slices, head=float(head),
                                          balance=float(balance), chunks=int(chunks) or None, exchange=exchange,
                                          keep_plain=keep_plain, colsplit=colsplit)
        slices = self.d.slices
        super().__init__(ctx, {"n_rows": n_rows, "nnz": nnz, "slices": slices, "head": head,
                               "chunks": self.d.chunks, "colsplit": self.d.colsplit}, "spmv", "GFLOP/s")
        x = ops.rand_uniform_(torch.empty(n_rows, device=ctx.device), 5, 0.0, 1.0)
        self.xp = self.d.to_padded(x)
        del x
        self.y = None
        # The column-split pipeline leaves each step's chunk-1 exchange in flight across the step boundary. Before it
        # is timed, the SAME job proves it on its own backend: ITERATE_STEPS chained steps x <- A x with the exchange
        # deferred must equal, bit for bit, the same steps with every exchange finished inside its step (same kernels,
        # same data: any difference is a missing wait). If they differ on any rank, the timed steps finish their
        # exchanges (defer off) and the line says so (pipeline_selftest False).
        self.defer, self.selftest = True, None
        if self.d.colsplit and ctx.distributed:
            a = self.d.iterate(self.xp, self.ITERATE_STEPS, defer=True).clone()
            b = self.d.iterate(self.xp, self.ITERATE_STEPS, defer=False)
            same = ctx.max_over_ranks(0.0 if torch.equal(a, b) else 1.0) == 0.0
            self.defer = self.selftest = same
            del a

    ITERATE_STEPS = 3

    def step(self):
        # the column-split pipeline: each step's last exchange overlaps the next step's first products (the next step
        # waits for it before the products that read those columns); check() finishes it
        self.y = self.d.step_padded(self.xp, defer_exchange=self.defer)

    def check(self, reduce: bool = True):
        """Every entry of the timed step's output layout (own rows AND the ghost entries the exchange wrote) against
        the fp64 product of its owner's row; then ITERATE_STEPS chained steps (each output the next input, exchanges
        deferred across step boundaries as in an iterating caller) against fp64 A^k x."""
        e = self.d.layout_max_rel_err(self.y, self.xp, reduce=reduce)
        self.y = None  # (iterate() reuses the output buffers)
        ei = self.d.iterate_max_rel_err(self.xp, self.ITERATE_STEPS, defer=self.defer, reduce=reduce)
        return {"max_rel_err_vs_fp64": e, "iterated_max_rel_err_vs_fp64": ei, "iterated_steps": self.ITERATE_STEPS,
                "pipeline_selftest": self.selftest, "deferred": self.defer and self.d.colsplit,
                "check_passed": e <= REL_ERR_LIMIT and ei <= REL_ERR_LIMIT}

    def compute_only_step(self):
        self.d.comm = False
        try:
            self.y = self.d.step_padded(self.xp, defer_exchange=self.defer)
        finally:
            self.d.comm = True

    def bytes_exchanged_per_step(self):
        return self.d.bytes_sent_per_step()

    def work_per_step(self):
        return 2.0 * self.d.local_nnz

    def report(self, seconds, steps):
        r = super().report(seconds, steps)
        nnz_all = self.d.local_nnz
        t = torch.tensor([float(nnz_all)], dtype=torch.float64, device=self.ctx.device)
        self.ctx.all_reduce_(t)
        r["value"] = 2.0 * t.item() * steps / seconds / 1e9  # strong scaling: fixed matrix, world-summed
        bytes_ = t.item() * 8 + self.d.n * 8 * 2
        r["effective_gbps"] = bytes_ * steps / seconds / 1e9
        return r


class Region3D(Workload):
    """3-D region growing on the reference volume (512^3, seed (50,300,300)), LDS-tiled kernel."""

    # T2: from the reference seed the region is exactly the box 0<x<100, 250<y<400, 250<z<400 of the
    # reference volume, whatever its noise background (ref 5-cuda-region-growing/raycast.cu:114-158, 281-318)
    BOX_VOXELS = 99 * 149 * 149  # 2,197,899

    def __init__(self, ctx, dim=512, method="tiled", **_):
        super().__init__(ctx, {"dim": dim}, "region3d", "Gvox/s")
        self.data = ops.create_volume(dim, device=ctx.device)
        self.method, self.region, self.launches = method, None, 0

    def step(self):
        self.region, self.launches = ops.region3d(self.data, method=self.method)

    def work_per_step(self):
        return float(self.data.numel())

    def check(self, reduce: bool = True):
        """The timed region: 2,197,899 voxels forming exactly the box (dim 512, the reference seed); other volume
        sizes against the serial CPU flood fill (csrc/cpu/oracles.c)."""
        got = self.region != 0
        voxels = int(got.sum())
        if self.data.shape[0] == 512:
            box = torch.zeros_like(got)
            box[251:400, 251:400, 1:100] = True  # [z][y][x]
            ok = voxels == self.BOX_VOXELS and torch.equal(got, box)
        else:
            ref, _ = ops.region3d(self.data.cpu())
            ok = torch.equal(got.cpu(), ref != 0)
        return {"region_voxels": voxels, "check_passed": bool(ok)}


class Raycast(Workload):
    def __init__(self, ctx, dim=512, image_dim=512, method="texture", **_):
        super().__init__(ctx, {"dim": dim, "image_dim": image_dim}, "raycast", "Grays/s")
        self.data = ops.create_volume(dim, device=ctx.device)
        self.region, _ = ops.region3d(self.data)
        self.image_dim, self.method = image_dim, method

    def step(self):
        self.image = ops.raycast(self.data, self.region, self.image_dim, method=self.method)

    def work_per_step(self):
        return float(self.image_dim ** 2)

    # texture path vs the global-memory caster (T5 image of the same volume): the texture path samples with
    # texel-centre addressing, correct weights and 8-bit fractional weights like a hardware filter (ref
    # raycast.cu:374-433 vs :321-371), so it agrees within a tolerance, not bit for bit
    TEX_MEAN_ABS_DIFF, TEX_MEAN_DIFF = 6.0, 3.0

    def check(self, reduce: bool = True):
        """texture: the timed image against the global-memory caster within the tolerance above; global: bit for
        bit against the serial CPU caster (ref raycast.cu:216-267) up to a 128^2 image (the 512^2 CPU oracle takes
        ~20 s), else against the global caster's own host-side rerun."""
        img = self.image.float()
        if self.method == "texture":
            ref = ops.raycast(self.data, self.region, self.image_dim, method="global").float()
            mad = (img - ref).abs().mean().item()
            md = abs(img.mean().item() - ref.mean().item())
            return {"mean_abs_diff_vs_global": mad, "mean_diff_vs_global": md,
                    "check_passed": mad < self.TEX_MEAN_ABS_DIFF and md < self.TEX_MEAN_DIFF}
        if self.image_dim <= 128 or not self.data.is_cuda:
            ref = ops.raycast(self.data.cpu(), self.region.cpu(), self.image_dim, method="global")
            return {"bit_exact_vs_cpu": bool(torch.equal(self.image.cpu(), ref)),
                    "check_passed": bool(torch.equal(self.image.cpu(), ref))}
        again = ops.raycast(self.data, self.region, self.image_dim, method=self.method)
        return {"deterministic": bool(torch.equal(again, self.image)), "check_passed": bool(torch.equal(again, self.image))}


class Histeq(Workload):
    def __init__(self, ctx, side=4096, **_):
        super().__init__(ctx, {"side": side}, "histeq", "Gpix/s")
        g = torch.Generator().manual_seed(7)
        self.img = torch.randint(0, 200, (side, side), dtype=torch.uint8, generator=g).to(ctx.device)

    def step(self):
        self.out = ops.histeq(self.img)

    def work_per_step(self):
        return float(self.img.numel())

    def check(self, reduce: bool = True):
        """Bit for bit against the serial host oracle (T3; ref 4-histogram-equalization-openmp-pthreads/
        histogram_serial.c:11-42)."""
        ref = ops.histeq(self.img.cpu(), method="serial")
        ok = torch.equal(self.out.cpu(), ref)
        return {"bit_exact_vs_serial": bool(ok), "check_passed": bool(ok)}


class Region2D(Workload):
    """The reference's MPI region-growing app on one device: corner-seeded 4-connected flood fill with
    |a-b| < 2 over pic1.bmp (ref 2-mpi-region-growing/region.c:493-533, 582-604). side > 512 tiles pic1 to
    side x side (longer propagation paths, more tiles); a step regrows from the seeds."""

    def __init__(self, ctx, side=512, **_):
        super().__init__(ctx, {"side": side}, "region2d", "Mpix/s")
        from pathlib import Path

        from ..utils import bmp

        self.assets = Path(__file__).resolve().parents[2] / "assets"
        pic = torch.from_numpy(bmp.read(self.assets / "pic1.bmp").copy())
        reps = max(1, -(-side // pic.shape[0]))
        self.img = pic.repeat(reps, reps)[:side, :side].contiguous().to(ctx.device)
        self.side = side

    def step(self):
        self.region = ops.region2d(self.img)

    def work_per_step(self):
        return float(self.img.numel())

    def scale(self):
        return 1e6

    def check(self, reduce: bool = True):
        """side 512: the output image (pixels of the region zeroed, ref region.c:572-580) equals the reference's
        golden out.bmp (T1, 64,420 region pixels); other sides: the region equals the serial CPU flood fill."""
        from ..utils import bmp

        reg = self.region.cpu() != 0
        if self.side == 512:
            golden = torch.from_numpy(bmp.read(self.assets / "region_pic1_golden.bmp").copy())
            out = self.img.cpu() * (~reg).to(torch.uint8)
            ok = torch.equal(out, golden)
            return {"region_pixels": int(reg.sum()), "golden_pixels": 64420, "matches_golden_bmp": bool(ok),
                    "check_passed": bool(ok)}
        ref = ops.region2d(self.img.cpu()) != 0
        ok = torch.equal(reg, ref)
        return {"region_pixels": int(reg.sum()), "matches_cpu_oracle": bool(ok), "check_passed": bool(ok)}


class Select(Workload):
    """Stream compaction of n f32 per GPU: keep the elements a mask (mode "mask": values, "index": their int32
    indices) or a predicate (mode "where": x < keep, no mask) selects, in order, with the count left on the device.
    x is uniform in [0, 1); the mask keeps element i when a seeded counter hash of i falls below the keep fraction.
    No communication (weak scaling)."""

    def __init__(self, ctx, n=1 << 28, keep=0.5, mode="mask", **_):
        if mode not in ("mask", "index", "where"):
            raise ValueError(f"select mode {mode!r}: mask, index or where")
        super().__init__(ctx, {"n": int(n), "keep": float(keep), "mode": mode}, "select", "GB/s")
        n, dev = int(n), ctx.device
        self.mode, self.keep = mode, float(keep)
        self.x = torch.empty(n, device=dev)
        ops.rand_uniform_(self.x, 7000 + ctx.rank, 0.0, 1.0)
        self.mask = None
        if mode != "where":
            u = ops.rand_uniform_(torch.empty(n, device=dev), 8000 + ctx.rank, 0.0, 1.0)  # the seeded counter
            self.mask = u < self.keep
            del u
        self.out = torch.empty(n, device=dev, dtype=torch.float32 if mode != "index" else torch.int32)
        self.count = None

    def step(self):
        if self.mode == "mask":
            _, self.count = ops.compact(self.x, self.mask, out=self.out)
        elif self.mode == "index":
            _, self.count = ops.compact_indices(self.mask, out=self.out)
        else:
            _, self.count = ops.compact_where(self.x, "lt", self.keep, out=self.out)

    def torch_step(self):
        """The same selection through torch (the vendor bar; it synchronises for the size of its result)."""
        if self.mode == "mask":
            return self.x[self.mask]
        if self.mode == "index":
            return torch.nonzero(self.mask)
        return self.x[self.x < self.keep]

    def kept(self) -> int:
        return int(self.count.item()) if self.count is not None else 0

    def work_per_step(self):
        # bytes moved: mask select reads 4n payload + n flags and writes 4k; index select reads the n flags alone;
        # the predicate reads the payload alone
        n, k = self.x.numel(), self.kept()
        return float({"mask": 5 * n, "index": n, "where": 4 * n}[self.mode] + 4 * k)

    def check(self, reduce: bool = True, chunk: int = 1 << 26):
        """Every output of the timed step and the count against torch (x[mask] / nonzero / x[x < keep]), bit for bit,
        chunk by chunk of the input; and the look-back error word of the stream. Local only."""
        lookback_ok = True
        if self.x.is_cuda:
            try:
                ops.scan_check(self.x.device)
            except RuntimeError:
                lookback_ok = False
        k, n, pos, same = self.kept(), self.x.numel(), 0, True
        for s in range(0, n, chunk):
            xs = self.x[s:s + chunk]
            keep = self.mask[s:s + chunk] if self.mode != "where" else xs < self.keep
            ref = (torch.nonzero(keep).reshape(-1) + s).int() if self.mode == "index" else xs[keep]
            m = ref.numel()
            same = same and pos + m <= k and torch.equal(self.out[pos:pos + m].view(torch.int32), ref.view(torch.int32))
            pos += m
        ok = bool(same and pos == k)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
            lookback_ok = self.ctx.max_over_ranks(0.0 if lookback_ok else 1.0) == 0.0
        return {"kept": k, "kept_torch": pos, "elements_checked": pos, "bit_exact_vs_torch": ok,
                "lookback_ok": lookback_ok, "check_passed": ok and lookback_ok}


class Sort(Workload):
    """Stable radix sort of n keys per GPU (csrc/kernels/sort.hip): mode "keys" (sorted keys), "pairs" (keys with an
    int32 payload) or "argsort" (int32 indices alone). dtype f32 (uniform in [-1, 1)) or i32 (uniform over the full range,
    or over [0, 2^bits) with bits=B, which then runs ceil(B / 8) passes); dist "equal" makes every key the same (every
    key in one digit bin: the worst case of the per-digit chain). No communication (weak scaling)."""

    def __init__(self, ctx, n=1 << 28, mode="keys", dtype="f32", bits=None, descending=False, dist="uniform", **_):
        if mode not in ("keys", "pairs", "argsort"):
            raise ValueError(f"sort mode {mode!r}: keys, pairs or argsort")
        if dtype not in ("f32", "i32"):
            raise ValueError(f"sort dtype {dtype!r}: f32 or i32")
        if dist not in ("uniform", "equal"):
            raise ValueError(f"sort dist {dist!r}: uniform or equal")
        bits = None if bits is None else int(bits)
        if bits is not None and dtype != "i32":
            raise ValueError("sort bits is for i32 keys only")
        super().__init__(ctx, {"n": int(n), "mode": mode, "dtype": dtype, "bits": bits, "descending": bool(descending),
                               "dist": dist}, "sort", "GB/s")
        n, dev = int(n), ctx.device
        self.mode, self.bits, self.descending = mode, bits, bool(descending)
        if dtype == "f32":
            self.x = ops.rand_uniform_(torch.empty(n, device=dev), 9000 + ctx.rank, -1.0, 1.0)
        else:
            g = torch.Generator(device=dev).manual_seed(9000 + ctx.rank)
            lo, hi = (0, 1 << bits) if bits is not None and bits < 32 else (-(1 << 31), 1 << 31)
            self.x = torch.randint(lo, hi, (n,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
        if dist == "equal":
            self.x.fill_(0.5 if dtype == "f32" else 1)
        self.payload = torch.arange(n, device=dev, dtype=torch.int32) if mode == "pairs" else None
        self.out = None

    def passes(self) -> int:
        return (32 if self.bits is None else self.bits) + 7 >> 3

    def step(self):
        kw = {"descending": self.descending, "bits": self.bits}
        if self.mode == "keys":
            self.out = (ops.sort_keys(self.x, **kw),)
        elif self.mode == "pairs":
            self.out = ops.sort_by_key(self.x, self.payload, **kw)
        else:
            self.out = (ops.argsort(self.x, **kw),)

    def torch_step(self):
        """The torch call each mode replaces (the vendor bar)."""
        if self.mode == "keys":
            return torch.sort(self.x, descending=self.descending).values
        r = torch.sort(self.x, stable=True, descending=self.descending)
        return r.indices if self.mode == "argsort" else r

    def work_per_step(self):
        # bytes moved: the histogram reads the keys once; a pass reads and writes 4 bytes per key, and 4 more each way
        # per value. An argsort's first pass reads no values (the index is computed), its last writes no keys.
        n, p = self.x.numel(), self.passes()
        per_pass = 8 if self.mode == "keys" else 16
        skipped = 8 if self.mode == "argsort" else 0
        return float(n * (4 + p * per_pass - skipped))

    def report(self, seconds: float, steps: int) -> dict:
        rep = super().report(seconds, steps)
        rep["gkeys_per_s"] = self.ctx.world * self.x.numel() * steps / seconds / 1e9
        rep["passes"] = self.passes()
        return rep

    def check(self, reduce: bool = True):
        """The outputs of the timed step against torch.sort(stable=True), exactly (indices and payload; keys bit for
        bit: the generated keys hold no NaN and no -0.0), and the look-back error word of the stream. Local only."""
        lookback_ok = True
        if self.x.is_cuda:
            try:
                ops.scan_check(self.x.device)
            except RuntimeError:
                lookback_ok = False
        ref = torch.sort(self.x, stable=True, descending=self.descending)
        same = True
        if self.mode != "argsort":
            same = torch.equal(self.out[0].view(torch.int32), ref.values.view(torch.int32))
        if self.mode != "keys":
            same = same and self.out[-1].dtype == torch.int32 and torch.equal(self.out[-1], ref.indices.int())
        ok = bool(same)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
            lookback_ok = self.ctx.max_over_ranks(0.0 if lookback_ok else 1.0) == 0.0
        return {"elements_checked": self.x.numel(), "exact_vs_torch": ok, "lookback_ok": lookback_ok,
                "check_passed": ok and lookback_ok}


class SegReduce(Workload):
    """Runs of equal neighbouring keys of n elements per GPU (csrc/kernels/segreduce.hip): mode "rle" (run keys and
    lengths of keys of dtype f32 / i32), "sum" (int32 keys, the values of dtype f32 / i32 summed per run) or "unique"
    (sorted distinct values and counts of an unsorted input: sort, then collapse). Element i starts a run when a seeded
    counter falls below 1 / mean_run, so run lengths are geometric with mean mean_run; mean_run=0 makes every key
    equal (one run across every tile). In "unique" the input is n draws from about n / mean_run values. No
    communication (weak scaling)."""

    def __init__(self, ctx, n=1 << 28, mean_run=4.0, mode="rle", dtype="f32", **_):
        if mode not in ("rle", "sum", "unique"):
            raise ValueError(f"segreduce mode {mode!r}: rle, sum or unique")
        if dtype not in ("f32", "i32"):
            raise ValueError(f"segreduce dtype {dtype!r}: f32 or i32")
        if float(mean_run) < 0 or 0 < float(mean_run) < 1:
            raise ValueError(f"segreduce mean_run {mean_run!r}: 0 (all keys equal) or >= 1")
        super().__init__(ctx, {"n": int(n), "mean_run": float(mean_run), "mode": mode, "dtype": dtype}, "segreduce", "GB/s")
        n, dev, mean_run = int(n), ctx.device, float(mean_run)
        self.mode = mode
        tdt = torch.float32 if dtype == "f32" else torch.int32
        u = ops.rand_uniform_(torch.empty(n, device=dev), 10000 + ctx.rank, 0.0, 1.0)  # the seeded counter
        if mode == "unique":
            groups = max(1, int(n / mean_run)) if mean_run else 1
            ids = (u.double() * groups).long().clamp_(max=groups - 1)
        else:
            ids = torch.cumsum(u < (1.0 / mean_run if mean_run else 0.0), 0)  # neighbouring runs get different ids
        del u
        ids = (ids % (1 << 24)).int()  # exact as float32 too (consecutive ids stay different)
        self.keys = ids.to(tdt) if mode != "sum" else ids
        del ids
        self.values = None
        if mode == "sum":
            v = ops.rand_uniform_(torch.empty(n, device=dev), 11000 + ctx.rank, 0.0, 1.0)
            self.values = v if dtype == "f32" else (v * 1000.0).int()
        self.out = None

    def step(self):
        if self.mode == "rle":
            self.out = ops.run_length_encode(self.keys)
        elif self.mode == "sum":
            self.out = ops.reduce_by_key(self.keys, self.values, "sum")
        else:
            rk, rc, num = ops.run_length_encode(ops.sort_keys(self.keys))
            self.out = (rk, rc, num)

    def torch_step(self):
        """The torch calls each mode replaces (the vendor bar; they synchronise for the size of their result)."""
        if self.mode == "rle":
            return torch.unique_consecutive(self.keys, return_counts=True)
        if self.mode == "sum":
            rk, inv = torch.unique_consecutive(self.keys, return_inverse=True)
            return rk, torch.zeros(rk.numel(), dtype=self.values.dtype, device=rk.device).index_add_(0, inv, self.values)
        return torch.unique(self.keys, return_counts=True)

    def runs(self) -> int:
        return int(self.out[-1].item()) if self.out is not None else 0

    def work_per_step(self):
        # bytes moved: the keys (and values) once, 8 bytes out per run; unique adds the sort's histogram read and four
        # read + write passes over the keys
        n, k = self.keys.numel(), self.runs()
        return float({"rle": 4 * n, "sum": 8 * n, "unique": (4 + 4 * 8 + 4) * n}[self.mode] + 8 * k)

    def _ref_chunks(self, chunk: int):
        """(key bits, per-run reference, chunk continues the previous run) of torch on each input chunk. The per-run
        reference is the int64 run length (rle) or the int64 / float64 sum (sum)."""
        n = self.keys.numel()
        kb = self.keys.view(torch.int32)
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            rk, inv, cnt = torch.unique_consecutive(kb[s:e], return_inverse=True, return_counts=True)
            if self.mode == "sum":
                acc = torch.float64 if self.values.dtype == torch.float32 else torch.int64
                cnt = torch.zeros(rk.numel(), dtype=acc, device=rk.device).index_add_(0, inv, self.values[s:e].to(acc))
            yield rk, cnt, bool(s > 0 and (kb[s] == kb[s - 1]).item())

    def _same(self, got: torch.Tensor, ref: torch.Tensor) -> bool:
        if ref.dtype == torch.float64:  # float32 sums: the fp64 sum of the same values, to REL_ERR_LIMIT
            return bool(((got.double() - ref).abs() <= REL_ERR_LIMIT * ref.abs().clamp_min(1.0)).all())
        return torch.equal(got.long(), ((ref + (1 << 31)) % (1 << 32)) - (1 << 31))  # int32 sums wrap

    def check(self, reduce: bool = True, chunk: int = 1 << 26):
        """Every output of the timed step against torch, chunk by chunk: run keys bit for bit and run lengths / int32
        sums exactly (runs that cross a chunk border are joined), float32 sums against the fp64 sums to REL_ERR_LIMIT,
        unique against torch.unique(return_counts=True); and the look-back error word of the stream. Local only."""
        lookback_ok = True
        if self.keys.is_cuda:
            try:
                ops.scan_check(self.keys.device)
            except RuntimeError:
                lookback_ok = False
        k, pos, same = self.runs(), 0, True
        okeys, oagg = self.out[0].view(torch.int32), self.out[1]
        if self.mode == "unique":
            rv, rc = torch.unique(self.keys, return_counts=True)
            pos = rv.numel()
            for s in range(0, pos if pos == k else 0, chunk):
                e = min(pos, s + chunk)
                same = same and torch.equal(okeys[s:e], rv.view(torch.int32)[s:e]) and torch.equal(oagg[s:e].long(), rc[s:e])
        else:
            pend_k = pend_v = None  # the last run of the chunks so far: it may go on in the next chunk
            for rk, rv, joins in self._ref_chunks(chunk):
                if pend_k is not None:
                    if joins:
                        rv[0] += pend_v[0]
                    else:
                        rk, rv = torch.cat([pend_k, rk]), torch.cat([pend_v, rv])
                m = rk.numel() - 1
                same = same and pos + m < k and torch.equal(okeys[pos:pos + m], rk[:m]) \
                    and self._same(oagg[pos:pos + m], rv[:m])
                pos += m
                pend_k, pend_v = rk[m:], rv[m:]
            if pend_k is not None:
                same = same and pos < k and torch.equal(okeys[pos:pos + 1], pend_k) and self._same(oagg[pos:pos + 1], pend_v)
                pos += 1
        ok = bool(same and pos == k)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
            lookback_ok = self.ctx.max_over_ranks(0.0 if lookback_ok else 1.0) == 0.0
        return {"runs": k, "runs_torch": pos, "elements_checked": self.keys.numel(), "matches_torch": ok,
                "lookback_ok": lookback_ok, "check_passed": ok and lookback_ok}


class ScanByKey(Workload):
    """The running op inside every run of n elements per GPU (csrc/kernels/scanbykey.hip): mode "keys"
    (ops.scan_by_key on int32 keys), "heads" (ops.segmented_scan on the bool head flags of the same runs) or "positions"
    (ops.run_positions: no values). op sum, min or max over values of dtype f32 (uniform in [0, 1)) or i32 (0..999),
    inclusive or exclusive. The runs are SegReduce's: element i starts one when a seeded counter falls below
    1 / mean_run (geometric lengths), mean_run=0 makes every key equal (the carry crosses every tile and the lead kernel
    rewrites the whole output). No communication (weak scaling)."""

    def __init__(self, ctx, n=1 << 28, mean_run=4.0, op="sum", dtype="f32", exclusive=False, mode="keys", **_):
        if mode not in ("keys", "heads", "positions"):
            raise ValueError(f"scanbykey mode {mode!r}: keys, heads or positions")
        if dtype not in ("f32", "i32"):
            raise ValueError(f"scanbykey dtype {dtype!r}: f32 or i32")
        if op not in ops.OP_CODES:
            raise ValueError(f"scanbykey op {op!r}: sum, min or max")
        if float(mean_run) < 0 or 0 < float(mean_run) < 1:
            raise ValueError(f"scanbykey mean_run {mean_run!r}: 0 (all keys equal) or >= 1")
        super().__init__(ctx, {"n": int(n), "mean_run": float(mean_run), "op": op, "dtype": dtype,
                               "exclusive": bool(exclusive), "mode": mode}, "scanbykey", "GB/s")
        n, dev, mean_run = int(n), ctx.device, float(mean_run)
        self.mode, self.op, self.exclusive = mode, op, bool(exclusive)
        u = ops.rand_uniform_(torch.empty(n, device=dev), 10000 + ctx.rank, 0.0, 1.0)  # the seeded counter
        head = u < (1.0 / mean_run if mean_run else 0.0)
        del u
        self.heads = head if mode == "heads" else None  # heads[0] may be 0: element 0 starts a run anyway
        self.keys = None if mode == "heads" else (torch.cumsum(head, 0) % (1 << 24)).int()  # neighbouring runs differ
        del head
        self.values = None
        if mode != "positions":
            v = ops.rand_uniform_(torch.empty(n, device=dev), 11000 + ctx.rank, 0.0, 1.0)
            self.values = v if dtype == "f32" else (v * 1000.0).int()
        self.out = None

    def step(self):
        if self.mode == "keys":
            self.out = ops.scan_by_key(self.keys, self.values, self.op, self.exclusive)
        elif self.mode == "heads":
            self.out = ops.segmented_scan(self.values, self.heads, self.op, self.exclusive)
        else:
            self.out = ops.run_positions(self.keys)

    def torch_step(self):
        """The torch composition this op replaces: run indices from unique_consecutive (or a cumsum of the flags), then
        a cumsum minus the gathered per-run base (float32 sums cancel), or a cummax over values lifted by
        4096 * run index for min / max (values below 1000 in magnitude, as here)."""
        if self.mode == "heads":
            h = self.heads.clone()
            h[:1] = True
            inv = torch.cumsum(h, 0) - 1
            starts = torch.nonzero(h).view(-1)
        else:
            _, inv, cnt = torch.unique_consecutive(self.keys, return_inverse=True, return_counts=True)
            starts = torch.cumsum(cnt, 0) - cnt
        if self.mode == "positions":
            return (torch.arange(inv.numel(), device=inv.device) - starts[inv]).int()
        v = self.values
        if self.op == "sum":
            c = torch.cumsum(v, 0, dtype=v.dtype)
            r = c - (c - v)[starts][inv]
            return r - v if self.exclusive else r
        sign = 1 if self.op == "max" else -1
        lift = inv.to(torch.float64 if v.dtype == torch.float32 else torch.int64) * 4096
        r = (sign * (torch.cummax(sign * v + lift, 0).values - lift)).to(v.dtype)
        if self.exclusive:
            ident = _scan_identity(self.op, v.dtype)
            r = torch.cat([r.new_full((1,), ident), r[:-1]])
            r[starts] = ident
        return r

    def work_per_step(self):
        # bytes moved once: keys or flag bytes, values, every output (the lead kernel's second pass is not counted)
        n = (self.keys if self.keys is not None else self.heads).numel()
        return float({"keys": 12, "heads": 9, "positions": 8}[self.mode] * n)

    def check(self, reduce: bool = True, chunk: int = 1 << 26):
        """Every output of the timed step against an exact oracle, chunk by chunk (a run that crosses a chunk border
        takes the previous chunk's last inclusive value as its carry): sums as an int64 / fp64 cumsum minus the gathered
        per-run base (int32 wrapped and compared exactly, float32 to REL_ERR_LIMIT of the fp64 value), min / max and
        positions exactly (a cummax over order-preserving int64 keys lifted by 2^33 * run index, so later runs
        dominate). Local only."""
        src = self.keys.view(torch.int32) if self.keys is not None else self.heads
        n, dev = src.numel(), src.device
        got_all = self.out.reshape(-1)
        same, carry, runs = True, None, 0
        is_f32 = self.mode != "positions" and self.values.dtype == torch.float32
        for s in range(0, n, chunk):
            e = min(n, s + chunk)
            m = e - s
            head = torch.ones(m, dtype=torch.bool, device=dev)
            if self.keys is not None:
                head[1:] = src[s + 1:e] != src[s:e - 1]
                joins = bool(s > 0 and (src[s] == src[s - 1]).item())
            else:
                head[1:] = src[s + 1:e] != 0
                joins = bool(s > 0 and (src[s] == 0).item())
            idx = torch.arange(m, device=dev)
            start = torch.cummax(torch.where(head, idx, 0), 0).values
            inv = torch.cumsum(head, 0) - 1
            runs += int(inv[-1].item()) + (0 if joins else 1)
            lead = (inv == 0) if joins else torch.zeros(m, dtype=torch.bool, device=dev)
            got = got_all[s:e]
            if self.mode == "positions":
                ref = idx - start
                if joins:
                    ref = ref + lead * carry
                carry = ref[-1] + 1
                same = same and torch.equal(got.long(), ref)
            elif self.op == "sum":
                acc = torch.float64 if is_f32 else torch.int64
                v = self.values[s:e].to(acc)
                c = torch.cumsum(v, 0)
                ref = c - (c - v)[start]
                if joins:
                    ref = ref + lead * carry
                carry = ref[-1]
                if self.exclusive:
                    ref = ref - v
                if is_f32:
                    same = same and bool(((got.double() - ref).abs() <= REL_ERR_LIMIT * ref.abs().clamp_min(1.0)).all())
                else:
                    same = same and torch.equal(got.long(), ((ref + (1 << 31)) % (1 << 32)) - (1 << 31))
            else:
                sign = 1 if self.op == "max" else -1
                ident = _ordered_i64(torch.full((1,), _scan_identity(self.op, got.dtype), dtype=got.dtype, device=dev))
                lift = inv << 33
                ref = sign * (torch.cummax(sign * _ordered_i64(self.values[s:e]) + lift, 0).values - lift)
                if joins:
                    ref = torch.where(lead, torch.maximum(sign * ref, sign * carry) * sign, ref)
                prev, carry = carry, ref[-1:].clone()
                if self.exclusive:
                    ref = torch.cat([prev if joins else ident, ref[:-1]])
                    ref[1:] = torch.where(head[1:], ident, ref[1:])
                same = same and torch.equal(_ordered_i64(got), ref)
        ok = bool(same)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"runs": runs, "elements_checked": n, "matches_oracle": ok, "check_passed": ok}


def _scan_identity(op: str, dtype: torch.dtype):
    if dtype == torch.float32:
        return {"sum": 0.0, "min": float("inf"), "max": float("-inf")}[op]
    return {"sum": 0, "min": 2**31 - 1, "max": -2**31}[op]


def _ordered_i64(t: torch.Tensor) -> torch.Tensor:
    """int64 keys in the order of the values of an int32 or NaN-free float32 tensor (the two zeros share a key)."""
    if t.dtype != torch.float32:
        return t.long()
    b = t.contiguous().view(torch.int32).long()
    return torch.where(b >= 0, b, -(b & 0x7fffffff))


class TopK(Workload):
    """The k best of n keys per GPU and their indices (csrc/kernels/topk.hip): dtype f32 (uniform in [-1, 1)) or i32
    (uniform over the full range); dist "equal" makes every key the same (every key ties with the k-th: the gather
    takes the first k indices), "sorted" sorts the keys ascending (the best are the last, or with largest=False the
    first, tiles). method is ops.topk's (None, "select", "sort"). No communication (weak scaling)."""

    def __init__(self, ctx, n=1 << 28, k=1024, dtype="f32", largest=True, sorted=True, dist="uniform", method=None,
                 **_):
        if dtype not in ("f32", "i32"):
            raise ValueError(f"topk dtype {dtype!r}: f32 or i32")
        if dist not in ("uniform", "equal", "sorted"):
            raise ValueError(f"topk dist {dist!r}: uniform, equal or sorted")
        n, k, dev = int(n), int(k), ctx.device
        if not 0 <= k <= n:
            raise ValueError(f"topk k {k}: 0..{n}")
        super().__init__(ctx, {"n": n, "k": k, "dtype": dtype, "largest": bool(largest), "sorted": bool(sorted),
                               "dist": dist, "method": method}, "topk", "GB/s")
        self.k, self.largest, self.sorted, self.method = k, bool(largest), bool(sorted), method
        if dtype == "f32":
            self.x = ops.rand_uniform_(torch.empty(n, device=dev), 12000 + ctx.rank, -1.0, 1.0)
        else:
            g = torch.Generator(device=dev).manual_seed(12000 + ctx.rank)
            self.x = torch.randint(-(1 << 31), 1 << 31, (n,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
        if dist == "equal":
            self.x.fill_(0.5 if dtype == "f32" else 1)
        elif dist == "sorted":
            self.x = torch.sort(self.x).values
        self.out = None

    def step(self):
        self.out = ops.topk(self.x, self.k, self.largest, self.sorted, method=self.method)

    def torch_step(self):
        """The torch call this replaces (the vendor bar; its choice among ties is unspecified)."""
        return torch.topk(self.x, self.k, largest=self.largest, sorted=self.sorted)

    def work_per_step(self):
        # bytes the select route really reads and writes: four histogram passes and the gather read the keys once each;
        # the gather writes 8 bytes per survivor; the survivor sort reads them once for its histogram and reads and
        # writes them in each of its four passes
        n, k = self.x.numel(), self.k
        return float(5 * 4 * n + 8 * k + ((4 + 4 * 16) * k if self.sorted and k > 1 else 0))

    def report(self, seconds: float, steps: int) -> dict:
        rep = super().report(seconds, steps)
        rep["gkeys_per_s"] = self.ctx.world * self.x.numel() * steps / seconds / 1e9
        rep["k"] = self.k
        return rep

    def check(self, reduce: bool = True):
        """The outputs of the timed step against the first k entries of torch.sort(stable=True), exactly (sorted=False:
        those entries re-ordered by index; values bit for bit: the generated keys hold no NaN and no -0.0), and the
        look-back error word of the stream. Local only."""
        lookback_ok = True
        if self.x.is_cuda:
            try:
                ops.scan_check(self.x.device)
            except RuntimeError:
                lookback_ok = False
        ref = torch.sort(self.x, stable=True, descending=self.largest)
        rv, ri = ref.values[:self.k], ref.indices[:self.k]
        if not self.sorted:
            ri, o = torch.sort(ri)
            rv = rv[o]
        same = self.out[1].dtype == torch.int32 and torch.equal(self.out[1], ri.int()) \
            and torch.equal(self.out[0].view(torch.int32), rv.view(torch.int32))
        ok = bool(same)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
            lookback_ok = self.ctx.max_over_ranks(0.0 if lookback_ok else 1.0) == 0.0
        return {"elements_checked": self.x.numel(), "k": self.k, "exact_vs_torch": ok, "lookback_ok": lookback_ok,
                "check_passed": ok and lookback_ok}


class Bincount(Workload):
    """int32 counts of n samples per GPU in num_bins bins (csrc/kernels/bincount.hip): mode "bincount" (ops.bincount on
    i32 or u8 samples, weights none, i32 or f32), "histc" (ops.histc on f32 samples over [0, 1]) or "edges"
    (ops.histogram with num_bins + 1 evenly spaced edges over [0, 1], at most 8192 bins). dist: "uniform" over the
    bins, "equal" (every sample in the middle bin: the worst case for same-address atomics), "sorted" (uniform, then
    sorted ascending) or "zipf" (bin b with weight about 1 / (b + 1)). f32 samples sit at bin centres. u8 samples reach
    at most 256 bins. No communication (weak scaling)."""

    def __init__(self, ctx, n=1 << 28, num_bins=256, dist="uniform", dtype="i32", mode="bincount", weights="none", **_):
        if dist not in ("uniform", "equal", "sorted", "zipf"):
            raise ValueError(f"bincount dist {dist!r}: uniform, equal, sorted or zipf")
        if dtype not in ("i32", "u8", "f32") or mode not in ("bincount", "histc", "edges"):
            raise ValueError(f"bincount dtype {dtype!r} / mode {mode!r}: i32, u8 or f32 / bincount, histc or edges")
        if (mode == "bincount") == (dtype == "f32"):
            raise ValueError(f"bincount mode {mode!r} takes {'i32 or u8' if mode == 'bincount' else 'f32'} samples")
        if weights not in ("none", "i32", "f32") or (weights != "none" and mode != "bincount"):
            raise ValueError(f"bincount weights {weights!r}: none, i32 or f32, with mode bincount only")
        n, num_bins, dev = int(n), int(num_bins), ctx.device
        if num_bins < 1 or (mode == "edges" and num_bins > ops.vector.HIST_MAX_EDGE_BINS):
            raise ValueError(f"bincount num_bins {num_bins}: at least 1, at most 8192 in mode edges")
        super().__init__(ctx, {"n": n, "num_bins": num_bins, "dist": dist, "dtype": dtype, "mode": mode,
                               "weights": weights}, "bincount", "GB/s")
        self.mode, self.num_bins = mode, num_bins
        reach = min(num_bins, 256) if dtype == "u8" else num_bins  # the bins the samples are spread over
        u = ops.rand_uniform_(torch.empty(n, device=dev), 13000 + ctx.rank, 0.0, 1.0)
        if dist == "zipf":
            b = torch.exp(u * float(torch.log(torch.tensor(float(reach) + 1.0)))).long() - 1
        else:
            b = (u * reach).long()
        b.clamp_(0, reach - 1)
        del u
        if dist == "equal":
            b.fill_(reach // 2)
        elif dist == "sorted":
            b = torch.sort(b).values
        if dtype == "f32":
            self.x = ((b.float() + 0.5) / float(num_bins))
        else:
            self.x = b.to(torch.uint8 if dtype == "u8" else torch.int32)
        del b
        self.edges = torch.linspace(0.0, 1.0, num_bins + 1, device=dev) if mode == "edges" else None
        self.w = None
        if weights != "none":
            w = ops.rand_uniform_(torch.empty(n, device=dev), 14000 + ctx.rank, 0.0, 1.0)
            self.w = w if weights == "f32" else (w * 1000.0).int()
        self.out = None

    def step(self):
        if self.mode == "bincount":
            self.out = ops.bincount(self.x, self.num_bins, self.w)
        elif self.mode == "histc":
            self.out = ops.histc(self.x, self.num_bins, 0.0, 1.0)
        else:
            self.out = ops.histogram(self.x, self.edges)

    def torch_step(self):
        """The torch call this replaces: torch.bincount (int64 counts, float atomics with float weights), torch.histc
        (float counts), or bucketize + bincount for explicit edges (torch.histogram has no GPU kernel)."""
        if self.mode == "bincount":
            return torch.bincount(self.x, weights=self.w, minlength=self.num_bins)
        if self.mode == "histc":
            return torch.histc(self.x, self.num_bins, 0.0, 1.0)
        return torch.bincount((torch.bucketize(self.x, self.edges, right=True) - 1).clamp_(0, self.num_bins - 1),
                              minlength=self.num_bins)

    def work_per_step(self):
        return float(self.x.numel() * (self.x.element_size() + (4 if self.w is not None else 0)))  # bytes read once

    def report(self, seconds: float, steps: int) -> dict:
        rep = super().report(seconds, steps)
        rep["gsamples_per_s"] = self.ctx.world * self.x.numel() * steps / seconds / 1e9
        return rep

    def oracle_bins(self) -> torch.Tensor:
        """int64 bin of every sample that falls in a bin, by the ops' definitions written with separate torch ops."""
        x, nb = self.x.reshape(-1), self.num_bins
        if self.mode == "bincount":
            v = x.long()
            return v[(v >= 0) & (v < nb)]
        if self.mode == "histc":
            lo, hi = torch.tensor(0.0, device=x.device), torch.tensor(1.0, device=x.device)
            scale = torch.tensor(float(nb), dtype=torch.float32, device=x.device) / (hi - lo)
            v = x[(x >= lo) & (x <= hi)]
            return ((v - lo) * scale).to(torch.int64).clamp(max=nb - 1)
        v = x[(x >= self.edges[0]) & (x <= self.edges[-1])]
        return (torch.bucketize(v, self.edges, right=True) - 1).clamp(0, nb - 1)

    def check(self, reduce: bool = True):
        """The counts of the timed step against torch.bincount of the oracle bins, exactly (int32 weights: int64 sums
        wrapped to int32, exactly; float32 weights: every bin within (m - 1) * 2^-24 * sum|w| of the fp64 sum, m the
        samples of the bin, the bound of any summation order). Local only."""
        nb = self.num_bins
        b = self.oracle_bins()
        if self.w is None:
            ok = self.out.dtype == torch.int32 and torch.equal(self.out, torch.bincount(b, minlength=nb).int())
        else:
            v = self.x.reshape(-1).long()
            w = self.w.reshape(-1)[(v >= 0) & (v < nb)]
            if w.dtype == torch.int32:
                s = torch.zeros(nb, dtype=torch.int64, device=w.device).index_add_(0, b, w.long())
                ok = self.out.dtype == torch.int32 and torch.equal(self.out.long(), ((s + (1 << 31)) % (1 << 32)) - (1 << 31))
            else:
                z = torch.zeros(nb, dtype=torch.float64, device=w.device)
                s, sa = z.clone().index_add_(0, b, w.double()), z.clone().index_add_(0, b, w.double().abs())
                m = torch.bincount(b, minlength=nb).double()
                bound = (m - 1).clamp_min(0) * 2.0 ** -24 * sa
                ok = self.out.dtype == torch.float32 and bool(((self.out.double() - s).abs() <= bound).all())
        ok = bool(ok)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"samples_counted": int(b.numel()), "elements_checked": self.x.numel(), "exact_vs_torch": ok,
                "check_passed": ok}


class Merge(Workload):
    """Merge of two sorted key arrays, or a sorted search, over n keys per GPU in all (csrc/kernels/merge.hip). mode
    "keys" (ops.merge_keys), "pairs" (ops.merge_by_key with an int32 payload), "index" (ops.merge: keys and int32
    indices into the concatenation), "search" (ops.searchsorted, needles in random order) or "search_sorted" (sorted
    needles, values_sorted=True). split is the fraction of n that is a (merge) or the needles (search), the rest is b /
    the haystack; na and nb, when given, set the two sizes directly. dtype f32 (uniform in [-1, 1)) or i32 (full
    range). dist: "interleaved" (both sides drawn from the same range), "disjoint" (every key of a below every key of
    b) or "equal" (one key everywhere: every comparison is a tie). No communication (weak scaling)."""

    MODES = ("keys", "pairs", "index", "search", "search_sorted")

    def __init__(self, ctx, n=1 << 28, mode="keys", dtype="f32", dist="interleaved", split=0.5, descending=False,
                 right=False, na=None, nb=None, **_):
        if mode not in self.MODES:
            raise ValueError(f"merge mode {mode!r}: one of {', '.join(self.MODES)}")
        if dtype not in ("f32", "i32"):
            raise ValueError(f"merge dtype {dtype!r}: f32 or i32")
        if dist not in ("interleaved", "disjoint", "equal"):
            raise ValueError(f"merge dist {dist!r}: interleaved, disjoint or equal")
        if na is None or nb is None:
            if not 0.0 <= float(split) <= 1.0:
                raise ValueError(f"merge split {split!r}: a fraction in [0, 1]")
            na = int(round(int(n) * float(split)))
            nb = int(n) - na
        na, nb, dev = int(na), int(nb), ctx.device
        super().__init__(ctx, {"n": na + nb, "na": na, "nb": nb, "mode": mode, "dtype": dtype, "dist": dist,
                               "descending": bool(descending), "right": bool(right)}, "merge", "GB/s")
        self.mode, self.descending, self.right = mode, bool(descending), bool(right)
        self.search = mode.startswith("search")

        def keys(count, seed, half):
            """count random keys; half -1 / +1: from the lower / upper half of the range (dist disjoint), 0: all of it"""
            if dtype == "f32":
                lo, hi = (-1.0, 1.0) if half == 0 else ((-1.0, 0.0) if half < 0 else (0.0, 1.0))
                x = ops.rand_uniform_(torch.empty(count, device=dev), seed, lo, hi)
            else:
                lo, hi = (-(1 << 31), 1 << 31) if half == 0 else ((-(1 << 31), 0) if half < 0 else (0, 1 << 31))
                g = torch.Generator(device=dev).manual_seed(seed)
                x = torch.randint(lo, hi, (count,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
            if dist == "equal":
                x.fill_(0.5 if dtype == "f32" else 1)
            return x

        def sorted_(x):
            return torch.sort(x, descending=self.descending).values

        first = -1 if dist == "disjoint" else 0
        if self.descending:
            first = -first
        self.a = keys(na, 15000 + ctx.rank, first)
        if mode != "search":
            self.a = sorted_(self.a)
        self.b = sorted_(keys(nb, 16000 + ctx.rank, -first))
        self.va = torch.arange(na, device=dev, dtype=torch.int32) if mode == "pairs" else None
        self.vb = torch.arange(na, na + nb, device=dev, dtype=torch.int32) if mode == "pairs" else None
        self.out = None

    def step(self):
        if self.mode == "keys":
            self.out = (ops.merge_keys(self.a, self.b, self.descending),)
        elif self.mode == "pairs":
            self.out = ops.merge_by_key(self.a, self.va, self.b, self.vb, self.descending)
        elif self.mode == "index":
            self.out = ops.merge(self.a, self.b, self.descending)
        else:
            self.out = (ops.searchsorted(self.b, self.a, self.right, self.descending, self.mode == "search_sorted"),)

    def torch_step(self):
        """The call a user makes today: a sort of the concatenation, or torch.searchsorted (ascending sequences only:
        a descending one is searched through its flipped copy)."""
        if self.search:
            if not self.descending:
                return torch.searchsorted(self.b, self.a, right=self.right)
            return self.b.numel() - torch.searchsorted(self.b.flip(0), self.a, right=not self.right)
        cat = torch.cat([self.a, self.b])
        if self.mode == "keys":
            return torch.sort(cat, descending=self.descending).values
        if self.mode == "pairs":
            r = torch.sort(cat, stable=True, descending=self.descending)
            return r.values, torch.cat([self.va, self.vb])[r.indices]
        return torch.sort(cat, stable=True, descending=self.descending)

    def work_per_step(self):
        # bytes moved: a merge reads every key once and writes it once, 4 more each way per value, 4 more for an index;
        # the sorted search reads needles and haystack once and writes one int32 per needle; the general search is
        # counted as its needles read and results written (what it reads of the haystack depends on the needles)
        na, nb = self.a.numel(), self.b.numel()
        if self.mode == "search":
            return float(8 * na)
        if self.mode == "search_sorted":
            return float(4 * (na + nb) + 4 * na)
        return float((na + nb) * {"keys": 8, "pairs": 16, "index": 12}[self.mode])

    def report(self, seconds: float, steps: int) -> dict:
        rep = super().report(seconds, steps)
        rep["gkeys_per_s"] = self.ctx.world * (self.a.numel() + self.b.numel()) * steps / seconds / 1e9
        return rep

    def check(self, reduce: bool = True):
        """The outputs of the timed step against the torch oracle, exactly: the stable torch.sort of the concatenation
        (keys bit for bit, indices, payload), or torch.searchsorted (the generated keys hold no NaN). Local only."""
        if self.search:
            ref = self.torch_step().int()
            ok = self.out[0].dtype == torch.int32 and torch.equal(self.out[0], ref)
        else:
            ref = torch.sort(torch.cat([self.a, self.b]), stable=True, descending=self.descending)
            ok = torch.equal(self.out[0].view(torch.int32), ref.values.view(torch.int32))
            if self.mode != "keys":
                ok = ok and self.out[1].dtype == torch.int32 and torch.equal(self.out[1], ref.indices.int())
        ok = bool(ok)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"elements_checked": self.a.numel() + (0 if self.search else self.b.numel()), "exact_vs_torch": ok,
                "check_passed": ok}


class RowSort(Workload):
    """Row-wise sort / top-k / k-th value of a [rows, cols] matrix per GPU along its last dimension
    (csrc/kernels/rowsort.hip): mode "keys" (ops.sort_keys), "index" (ops.sort), "pairs" (ops.sort_by_key with the keys
    as their own payload), "topk" (ops.topk with k) or "kth" (ops.kth_value with k); dtype f32 (multiples of 1/64 from
    a normal distribution, so every row has ties) or i32 (the full range). route is the ops' (None picks by shape).
    No communication (weak scaling)."""

    MODES = ("keys", "index", "pairs", "topk", "kth")

    def __init__(self, ctx, rows=1 << 14, cols=4096, k=64, mode="keys", dtype="f32", descending=False, route=None, **_):
        if mode not in self.MODES:
            raise ValueError(f"rowsort mode {mode!r}: one of {self.MODES}")
        if dtype not in ("f32", "i32"):
            raise ValueError(f"rowsort dtype {dtype!r}: f32 or i32")
        rows, cols, k = int(rows), int(cols), int(k)
        if mode in ("topk", "kth") and not (1 if mode == "kth" else 0) <= k <= cols:
            raise ValueError(f"rowsort k {k}: at most cols = {cols}")
        super().__init__(ctx, {"rows": rows, "cols": cols, "k": k, "mode": mode, "dtype": dtype,
                               "descending": bool(descending), "route": route}, "rowsort", "GB/s")
        self.mode, self.k, self.descending, self.route = mode, k, bool(descending), route
        g = torch.Generator(device=ctx.device).manual_seed(16000 + ctx.rank)
        if dtype == "f32":
            self.x = torch.round(torch.randn(rows, cols, device=ctx.device, generator=g) * 64) / 64
        else:
            self.x = torch.randint(-(1 << 31), 1 << 31, (rows, cols), device=ctx.device, generator=g,
                                   dtype=torch.int64).to(torch.int32)
        self.out = None

    def step(self):
        x, d, r = self.x, self.descending, self.route
        if self.mode == "keys":
            self.out = (ops.sort_keys(x, d, dim=-1, route=r),)
        elif self.mode == "index":
            self.out = ops.sort(x, d, dim=-1, route=r)
        elif self.mode == "pairs":
            self.out = ops.sort_by_key(x, x, d, dim=-1, route=r)
        elif self.mode == "topk":
            self.out = ops.topk(x, self.k, largest=d, dim=-1, route=r)
        else:
            self.out = (ops.kth_value(x, self.k, largest=d, dim=-1),)

    def torch_step(self):
        """The torch call this replaces (the vendor bar)."""
        if self.mode == "topk":
            return torch.topk(self.x, self.k, dim=-1, largest=self.descending)
        if self.mode == "kth":
            return torch.kthvalue(self.x, self.k if not self.descending else self.x.shape[1] - self.k + 1, dim=-1)
        return torch.sort(self.x, dim=-1, stable=True, descending=self.descending)

    def work_per_step(self):
        # the bytes a caller sees move: the keys read once, and what is written
        n, kept = self.x.numel(), self.x.shape[0] * self.k
        return float({"keys": 8 * n, "index": 12 * n, "pairs": 16 * n, "topk": 4 * n + 8 * kept,
                      "kth": 4 * n + 4 * self.x.shape[0]}[self.mode])

    def report(self, seconds: float, steps: int) -> dict:
        rep = super().report(seconds, steps)
        rep["gkeys_per_s"] = self.ctx.world * self.x.numel() * steps / seconds / 1e9
        return rep

    def check(self, reduce: bool = True):
        """The outputs of the timed step against torch.sort(dim=-1, stable=True) of a host copy, exactly (values bit
        for bit: the generated keys hold no NaN; a -0.0 comes out as +0.0 on both sides). Local only."""
        xh = self.x.cpu()
        ref = torch.sort(xh, dim=-1, stable=True, descending=self.descending)
        rv = torch.where(ref.values == 0, torch.zeros_like(ref.values), ref.values)
        ri = ref.indices.int()
        out = [t.cpu() for t in self.out]
        same = lambda a, b: a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
        if self.mode == "keys":
            ok = same(out[0], rv)
        elif self.mode == "index":
            ok = same(out[0], rv) and same(out[1], ri)
        elif self.mode == "pairs":
            ok = same(out[0], rv) and same(out[1], torch.gather(xh.view(torch.int32), 1, ref.indices).view(xh.dtype))
        elif self.mode == "topk":
            ok = same(out[0], rv[:, :self.k]) and same(out[1], ri[:, :self.k])
        else:
            ok = same(out[0], rv[:, self.k - 1])
        ok = bool(ok)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"elements_checked": self.x.numel(), "exact_vs_torch": ok, "check_passed": ok}


class Axis(Workload):
    """Reduce or scan along the middle extent of an [outer, n, inner] tensor per GPU (csrc/kernels/axis.hip): mode
    "reduce" (ops.reduce(x, op, dim=1)) or "scan" (ops.scan(x, exclusive, dim=1, op=op)); op sum / min / max; dtype f32
    (whole numbers in [-8, 8], or in [-1, 1] for n above 2^20, so a sum is exact in any order up to n = 2^24) or i32
    (the full range: sums wrap). inner == 1 is the last-dimension case. route and chunk are the ops' (None picks by
    shape). No communication (weak scaling)."""

    MODES = ("reduce", "scan")

    def __init__(self, ctx, outer=1 << 14, n=4096, inner=1, mode="reduce", op="sum", dtype="f32", exclusive=False,
                 route=None, chunk=None, **_):
        if mode not in self.MODES:
            raise ValueError(f"axis mode {mode!r}: one of {self.MODES}")
        if op not in ops.OP_CODES:
            raise ValueError(f"axis op {op!r}: one of {sorted(ops.OP_CODES)}")
        if dtype not in ("f32", "i32"):
            raise ValueError(f"axis dtype {dtype!r}: f32 or i32")
        outer, n, inner = int(outer), int(n), int(inner)
        if min(outer, n, inner) < 1:
            raise ValueError(f"axis shape [{outer}, {n}, {inner}]: every extent at least 1")
        super().__init__(ctx, {"outer": outer, "n": n, "inner": inner, "mode": mode, "op": op, "dtype": dtype,
                               "exclusive": bool(exclusive), "route": route, "chunk": chunk}, "axis", "GB/s")
        self.mode, self.op, self.exclusive, self.route, self.chunk = mode, op, bool(exclusive), route, chunk
        g = torch.Generator(device=ctx.device).manual_seed(17000 + ctx.rank)
        amp = 8 if n <= 1 << 20 else 1
        self.x = torch.randint(-amp if dtype == "f32" else -(1 << 31), amp + 1 if dtype == "f32" else 1 << 31,
                               (outer, n, inner), device=ctx.device, generator=g, dtype=torch.int64)
        self.x = self.x.float() if dtype == "f32" else self.x.to(torch.int32)
        self.exact = dtype == "i32" or op != "sum" or amp * n < 1 << 24
        self.out = None
        _axis_plan(mode, route, chunk, outer, n, inner, "axis")  # a route that cannot take the shape raises here

    def step(self):
        if self.mode == "reduce":
            self.out = ops.reduce(self.x, self.op, dim=1, route=self.route, chunk=self.chunk)
        else:
            self.out = ops.scan(self.x, self.exclusive, dim=1, op=self.op, route=self.route, chunk=self.chunk)

    def torch_step(self):
        """The torch call this replaces (the vendor bar)."""
        if self.mode == "reduce":
            return {"sum": torch.sum, "min": torch.amin, "max": torch.amax}[self.op](self.x, 1)
        if self.op == "sum":
            return torch.cumsum(self.x, 1, dtype=self.x.dtype)
        return (torch.cummin if self.op == "min" else torch.cummax)(self.x, 1).values

    def work_per_step(self):
        # the bytes a caller sees move: the input read once, and what is written
        out = self.x.numel() if self.mode == "scan" else self.x.shape[0] * self.x.shape[2]
        return float(4 * (self.x.numel() + out))

    def check(self, reduce: bool = True):
        """Every output of the timed step against the host path of the same op on a host copy: exactly, except a
        float32 sum of more than 2^24 terms' worth of magnitude, which is held to the bound of any summation order,
        terms * 2^-24 * sum |x|. Local only."""
        xh, out = self.x.cpu(), self.out.cpu()
        ref = ops.reduce(xh, self.op, dim=1) if self.mode == "reduce" else ops.scan(xh, self.exclusive, dim=1, op=self.op)
        ok = out.dtype == ref.dtype and out.shape == ref.shape
        if ok and self.exact:
            ok = torch.equal(out, ref)
        elif ok:
            mag = xh.abs().double()
            mag = mag.sum(1) if self.mode == "reduce" else torch.cumsum(mag, 1)
            ok = bool(((out.double() - ref.double()).abs() <= xh.shape[1] * 2.0 ** -24 * mag).all())
        ok = bool(ok)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"elements_checked": self.out.numel(), "exact_vs_host": bool(self.exact), "check_passed": ok}

    def report(self, seconds: float, steps: int) -> dict:
        rep = super().report(seconds, steps)
        rep["gelems_per_s"] = self.ctx.world * self.x.numel() * steps / seconds / 1e9
        return rep


class Ragged(Workload):
    """Reduction over ragged segments given by offsets (csrc/kernels/ragged.hip): ops.segment_reduce(x, offsets, op) on
    n elements per GPU. dist places the segment borders: "uniform" (n / mean_len borders drawn uniformly: lengths vary,
    some segments are empty), "equal" (every segment mean_len long, the last one with the remainder), "powerlaw" (the row lengths of
    ops.sparse.powerlaw_row_ptr, the SpMV matrices' rows) or "empty" (S = 4 n: most segments are empty). op sum / min /
    max; dtype f32 (whole numbers in [-8, 8], or in [-1, 1] when the longest segment could otherwise leave the exact
    range) or i32 (the full range: sums wrap). No communication (weak scaling)."""

    DISTS = ("uniform", "equal", "powerlaw", "empty")

    def __init__(self, ctx, n=1 << 28, mean_len=100.0, dist="uniform", op="sum", dtype="f32", **_):
        if dist not in self.DISTS:
            raise ValueError(f"ragged dist {dist!r}: one of {self.DISTS}")
        if op not in ops.OP_CODES:
            raise ValueError(f"ragged op {op!r}: one of {sorted(ops.OP_CODES)}")
        if dtype not in ("f32", "i32"):
            raise ValueError(f"ragged dtype {dtype!r}: f32 or i32")
        n, mean_len = int(n), float(mean_len)
        if n < 1 or mean_len < 1.0:
            raise ValueError(f"ragged n = {n}, mean_len = {mean_len}: both at least 1")
        super().__init__(ctx, {"n": n, "mean_len": mean_len, "dist": dist, "op": op, "dtype": dtype}, "ragged", "GB/s")
        self.op = op
        dev = ctx.device
        g = torch.Generator(device=dev).manual_seed(18000 + ctx.rank)
        s = 4 * n if dist == "empty" else max(1, int(n / mean_len))
        if dist == "equal":
            off = torch.clamp(torch.arange(s + 1, device=dev, dtype=torch.int64) * int(mean_len), max=n)
            off[-1] = n  # the last segment takes the remainder
        elif dist == "powerlaw":
            off = torch.clamp(powerlaw_row_ptr(s, n, seed=18 + ctx.rank), max=n).to(dev)
        else:
            cuts = torch.sort(torch.randint(0, n + 1, (s - 1,), device=dev, generator=g, dtype=torch.int32)).values
            off = torch.cat([cuts.new_zeros(1), cuts, cuts.new_full((1,), n)])
        self.offsets = off.to(torch.int32).contiguous()
        self.offsets64 = None  # torch_step's copy, made on first use
        longest = int((self.offsets[1:] - self.offsets[:-1]).max())
        amp = 8 if 8 * longest < 1 << 24 else 1
        self.exact = dtype == "i32" or op != "sum" or amp * longest < 1 << 24
        self.x = torch.randint(-amp if dtype == "f32" else -(1 << 31), amp + 1 if dtype == "f32" else 1 << 31, (n,),
                               device=dev, generator=g, dtype=torch.int64)
        self.x = self.x.float() if dtype == "f32" else self.x.to(torch.int32)
        self.out = None

    def segments(self) -> int:
        return self.offsets.numel() - 1

    def step(self):
        self.out = ops.segment_reduce(self.x, self.offsets, self.op)

    def torch_step(self):
        """The torch call this replaces (the vendor bar); torch.segment_reduce takes floating types only."""
        if self.offsets64 is None:
            self.offsets64 = self.offsets.long()
        return torch.segment_reduce(self.x, self.op, offsets=self.offsets64)

    def work_per_step(self):
        # the bytes a caller sees move: the elements and the offsets read once, one result per segment written
        return float(4 * (self.x.numel() + 2 * self.segments() + 1))

    def check(self, reduce: bool = True):
        """Every result of the timed step against the host path on a host copy: exactly, except a float32 sum whose
        longest segment could leave the exact range, which is held to twice the bound of any summation order, terms *
        2^-24 * sum |x| per segment (the host path sums in float32 too). Local only."""
        xh, oh, out = self.x.cpu(), self.offsets.cpu(), self.out.cpu()
        ref = ops.segment_reduce(xh, oh, self.op)
        ok = out.dtype == ref.dtype and out.shape == ref.shape
        if ok and self.exact:
            ok = torch.equal(out, ref)
        elif ok:
            mag = ops.segment_reduce(xh.abs(), oh, "sum").double()
            terms = (oh[1:] - oh[:-1]).double()
            ok = bool(((out.double() - ref.double()).abs() <= 2.0 * terms * 2.0 ** -24 * mag).all())  # both are float32 sums
        ok = bool(ok)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"elements_checked": self.out.numel(), "exact_vs_host": bool(self.exact), "check_passed": ok}

    def report(self, seconds: float, steps: int) -> dict:
        rep = super().report(seconds, steps)
        rep["gelems_per_s"] = self.ctx.world * self.x.numel() * steps / seconds / 1e9
        rep["segments"] = self.segments()
        return rep


class SegSort(Ragged):
    """Sort inside ragged segments given by offsets (csrc/kernels/segsort.hip) on n keys per GPU: mode "keys"
    (ops.segment_sort_keys), "index" (ops.segment_sort) or "pairs" (ops.segment_sort_by_key with the keys as their own
    payload). dist places the segment borders as in the ragged workload ("uniform", "equal", "powerlaw", "empty"); dtype
    f32 (multiples of 1/64 from a normal distribution, so every longer segment has ties) or i32 (the full range). route
    and max_len are the ops'. No communication (weak scaling)."""

    MODES = ("keys", "index", "pairs")

    def __init__(self, ctx, n=1 << 28, mean_len=100.0, dist="uniform", mode="keys", dtype="f32", descending=False,
                 route=None, max_len=None, **_):
        if mode not in self.MODES:
            raise ValueError(f"segsort mode {mode!r}: one of {self.MODES}")
        Ragged.__init__(self, ctx, n, mean_len, dist, "min", dtype)  # the offsets; x is replaced below
        self.name = "segsort"
        self.cfg = {"n": int(n), "mean_len": float(mean_len), "dist": dist, "mode": mode, "dtype": dtype,
                    "descending": bool(descending), "route": route, "max_len": max_len}
        self.mode, self.descending, self.route = mode, bool(descending), route
        self.max_len = None if max_len is None else int(max_len)
        g = torch.Generator(device=ctx.device).manual_seed(20000 + ctx.rank)
        if dtype == "f32":
            self.x = torch.round(torch.randn(int(n), device=ctx.device, generator=g) * 64) / 64
        else:
            self.x = torch.randint(-(1 << 31), 1 << 31, (int(n),), device=ctx.device, generator=g,
                                   dtype=torch.int64).to(torch.int32)
        self.seg_ids = None  # torch_step's segment ids, made on first use

    def _run(self, x, offsets):
        kw = dict(descending=self.descending, route=self.route, max_len=self.max_len)
        if self.mode == "keys":
            return (ops.segment_sort_keys(x, offsets, **kw),)
        if self.mode == "index":
            return ops.segment_sort(x, offsets, **kw)
        return ops.segment_sort_by_key(x, x, offsets, **kw)

    def step(self):
        self.out = self._run(self.x, self.offsets)

    def torch_step(self):
        """What a torch caller composes (the vendor bar): a stable sort of the keys, then a stable sort of the segment
        ids (keys behind the last offset form one more group: the same work)."""
        if self.seg_ids is None:
            self.seg_ids = torch.searchsorted(self.offsets.long(), torch.arange(self.x.numel(), device=self.x.device),
                                              right=True)
        v, i = torch.sort(self.x, stable=True, descending=self.descending)
        order = i[torch.sort(self.seg_ids[i], stable=True).indices]
        return self.x[order], order

    def work_per_step(self):
        # the bytes a caller sees move: the keys and the offsets read once, and what is written
        n = self.x.numel()
        return float({"keys": 8 * n, "index": 12 * n, "pairs": 16 * n}[self.mode] + 4 * (self.segments() + 1))

    def check(self, reduce: bool = True):
        """Every output of the timed step against the host path of the same op on a host copy, bit for bit. Local only."""
        ref = self._run(self.x.cpu(), self.offsets.cpu())
        out = [t.cpu() for t in self.out]
        ok = len(out) == len(ref) and all(a.dtype == b.dtype and a.shape == b.shape and
                                          torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(out, ref))
        ok = bool(ok)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"elements_checked": self.x.numel(), "exact_vs_host": True, "check_passed": ok}

    def report(self, seconds: float, steps: int) -> dict:
        rep = Workload.report(self, seconds, steps)
        rep["gkeys_per_s"] = self.ctx.world * self.x.numel() * steps / seconds / 1e9
        rep["segments"] = self.segments()
        return rep


class ArgReduce(Workload):
    """argmin / argmax (csrc/kernels/argreduce.hip) per GPU: form "flat" (ops.arg_reduce(x, op) on n elements), "dim"
    (ops.arg_reduce(x, op, dim=1) on an [outer, n, inner] tensor, route and chunk the op's) or "segments"
    (ops.segment_arg_reduce(x, offsets, op) on n elements, dist and mean_len placing the borders as in the ragged
    workload). op max / min; dtype f32 (multiples of 1/4 from a normal distribution, so longer rows hold their
    extremum several times) or i32 (the full range). No communication (weak scaling)."""

    FORMS = ("flat", "dim", "segments")

    def __init__(self, ctx, form="flat", op="max", dtype="f32", n=1 << 28, outer=1 << 14, inner=1, route=None, chunk=None,
                 mean_len=100.0, dist="uniform", **_):
        if form not in self.FORMS:
            raise ValueError(f"argreduce form {form!r}: one of {self.FORMS}")
        if op not in ops.vector.ARG_OPS:
            raise ValueError(f"argreduce op {op!r}: one of {ops.vector.ARG_OPS}")
        if dtype not in ("f32", "i32"):
            raise ValueError(f"argreduce dtype {dtype!r}: f32 or i32")
        n, outer, inner = int(n), int(outer), int(inner)
        if min(outer, n, inner) < 1:
            raise ValueError(f"argreduce n = {n}, outer = {outer}, inner = {inner}: every extent at least 1")
        if form != "dim" and (route is not None or chunk is not None):
            raise ValueError("argreduce: route and chunk go with form 'dim'")
        super().__init__(ctx, {"form": form, "op": op, "dtype": dtype, "n": n}, "argreduce", "GB/s")
        self.form, self.op, self.route, self.chunk, self.offsets = form, op, route, chunk, None
        shape = (n,)
        if form == "dim":
            shape = (outer, n, inner)
            self.cfg.update({"outer": outer, "inner": inner, "route": route, "chunk": chunk})
            _axis_plan("reduce", route, chunk, outer, n, inner, "argreduce")  # a route that cannot take the shape raises here
        elif form == "segments":
            self.cfg.update({"mean_len": float(mean_len), "dist": dist})
            self.offsets = Ragged(ctx, n, mean_len, dist, "max", "i32").offsets
        g = torch.Generator(device=ctx.device).manual_seed(23000 + ctx.rank)
        if dtype == "f32":
            self.x = torch.round(torch.randn(shape, device=ctx.device, generator=g) * 4) / 4
        else:
            self.x = torch.randint(-(1 << 31), 1 << 31, shape, device=ctx.device, generator=g, dtype=torch.int64).to(torch.int32)
        self.out = None

    def _run(self, x, offsets):
        if self.form == "flat":
            return ops.arg_reduce(x, self.op)
        if self.form == "dim":
            return ops.arg_reduce(x, self.op, dim=1, route=self.route, chunk=self.chunk)
        return ops.segment_arg_reduce(x, offsets, self.op)

    def step(self):
        self.out = self._run(self.x, self.offsets)

    def torch_step(self):
        """The torch call this replaces (the vendor bar); torch has no arg form of segment_reduce."""
        if self.form == "flat":
            return torch.argmax(self.x) if self.op == "max" else torch.argmin(self.x)
        if self.form == "dim":
            return (torch.max if self.op == "max" else torch.min)(self.x, 1)
        raise NotImplementedError("torch has no argmax over ragged segments")

    def results(self) -> int:
        return 1 if self.form == "flat" else (self.x.shape[0] * self.x.shape[2] if self.form == "dim" else self.offsets.numel() - 1)

    def work_per_step(self):
        # the bytes a caller sees move: the input (and the offsets) read once, a value and an index per result written
        offs = 0 if self.offsets is None else self.offsets.numel()
        return float(4 * (self.x.numel() + offs + 2 * self.results()))

    def check(self, reduce: bool = True):
        """Values (as bit patterns) and indices of the timed step against the host path on a host copy. Local only."""
        ref = self._run(self.x.cpu(), None if self.offsets is None else self.offsets.cpu())
        out = [t.cpu() for t in self.out]
        ok = all(a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))
                 for a, b in zip(out, ref))
        ok = bool(ok)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"elements_checked": 2 * self.results(), "exact_vs_host": True, "check_passed": ok}

    def report(self, seconds: float, steps: int) -> dict:
        rep = super().report(seconds, steps)
        rep["gelems_per_s"] = self.ctx.world * self.x.numel() * steps / seconds / 1e9
        rep["results"] = self.results()
        return rep


class SetOps(Workload):
    """A set operation on two sorted key arrays of n keys per GPU in all (csrc/kernels/setops.hip): op intersection,
    union, difference or symmetric_difference; mode "keys" (ops.set_compact), "index" (keys and int32 indices into the
    concatenation) or "pairs" (ops.set_compact_by_key with an int32 payload). split is the fraction of n that is a.
    dtype f32 (uniform in [-1, 1)) or i32 (full range). dist: "interleaved" (both sides drawn from the same range),
    "disjoint" (every key of a below every key of b), "identical" (both sides are prefixes of one sorted array: equal
    sides at split 0.5), "ties" (eight distinct keys) or "equal" (one key everywhere). The timed step does not
    synchronise: the count stays on the device. No communication (weak scaling)."""

    MODES = ("keys", "index", "pairs")
    DISTS = ("interleaved", "disjoint", "identical", "ties", "equal")

    def __init__(self, ctx, n=1 << 28, op="intersection", mode="keys", dtype="f32", dist="interleaved", split=0.5,
                 descending=False, **_):
        if op not in SET_OP_CODES:
            raise ValueError(f"setops op {op!r}: one of {', '.join(SET_OP_CODES)}")
        if mode not in self.MODES:
            raise ValueError(f"setops mode {mode!r}: one of {', '.join(self.MODES)}")
        if dtype not in ("f32", "i32"):
            raise ValueError(f"setops dtype {dtype!r}: f32 or i32")
        if dist not in self.DISTS:
            raise ValueError(f"setops dist {dist!r}: one of {', '.join(self.DISTS)}")
        if not 0.0 <= float(split) <= 1.0:
            raise ValueError(f"setops split {split!r}: a fraction in [0, 1]")
        na = int(round(int(n) * float(split)))
        nb, dev = int(n) - na, ctx.device
        super().__init__(ctx, {"n": na + nb, "na": na, "nb": nb, "op": op, "mode": mode, "dtype": dtype, "dist": dist,
                               "descending": bool(descending)}, "setops", "GB/s")
        self.op, self.mode, self.descending = op, mode, bool(descending)

        def keys(count, seed, half):
            """count sorted keys; half -1 / +1: from the lower / upper half of the range (dist disjoint), 0: all of it"""
            g = torch.Generator(device=dev).manual_seed(seed)
            if dist == "ties":
                x = torch.randint(0, 8, (count,), device=dev, generator=g).to(torch.float32 if dtype == "f32" else torch.int32)
            elif dtype == "f32":
                lo, hi = (-1.0, 1.0) if half == 0 else ((-1.0, 0.0) if half < 0 else (0.0, 1.0))
                x = ops.rand_uniform_(torch.empty(count, device=dev), seed, lo, hi)
            else:
                lo, hi = (-(1 << 31), 1 << 31) if half == 0 else ((-(1 << 31), 0) if half < 0 else (0, 1 << 31))
                x = torch.randint(lo, hi, (count,), device=dev, generator=g, dtype=torch.int64).to(torch.int32)
            if dist == "equal":
                x.fill_(0.5 if dtype == "f32" else 1)
            return torch.sort(x, descending=self.descending).values

        if dist == "identical":
            both = keys(max(na, nb), 17000 + ctx.rank, 0)
            self.a, self.b = both[:na].clone(), both[:nb].clone()
        else:
            first = (-1 if dist == "disjoint" else 0) * (-1 if self.descending else 1)
            self.a, self.b = keys(na, 17000 + ctx.rank, first), keys(nb, 18000 + ctx.rank, -first)
        self.va = torch.arange(na, device=dev, dtype=torch.int32) if mode == "pairs" else None
        self.vb = torch.arange(na, na + nb, device=dev, dtype=torch.int32) if mode == "pairs" else None
        self.out = None

    def step(self):
        if self.mode == "pairs":
            self.out = ops.set_compact_by_key(self.a, self.va, self.b, self.vb, self.op, self.descending)
        else:
            self.out = ops.set_compact(self.a, self.b, self.op, self.descending, indices=self.mode == "index")

    def reference(self) -> torch.Tensor:
        """int64 positions in cat(a, b) of the kept elements in merge order, from the stable torch.sort of the
        concatenation and its runs of equal keys (the generated keys hold no NaN): inside a run come the m elements
        of a, then the n of b, and the i-th of each side are partners."""
        cat = torch.cat([self.a, self.b])
        na = self.a.numel()
        r = torch.sort(cat, stable=True, descending=self.descending)
        _, run, length = torch.unique_consecutive(r.values, return_inverse=True, return_counts=True)
        from_a = r.indices < na
        m = torch.zeros_like(length).scatter_add_(0, run, from_a.long())
        start = torch.cumsum(length, 0) - length
        place = torch.arange(cat.numel(), device=cat.device) - start[run]  # place in the run
        paired = torch.where(from_a, place < (length - m)[run], place - m[run] < m[run])
        keep = {"intersection": from_a & paired, "union": from_a | ~paired, "difference": from_a & ~paired,
                "symmetric_difference": ~paired}[self.op]
        return r.indices[keep]

    def work_per_step(self):
        # bytes moved: both inputs are read once (4 more per key for a payload), every kept element is written once
        # (4 more for its value or index). The kept count is that of the last step (one sync, after the timed window).
        n = self.a.numel() + self.b.numel()
        kept = int(self.out[-1].item()) if self.out is not None else 0
        return float(n * (8 if self.mode == "pairs" else 4) + kept * (4 if self.mode == "keys" else 8))

    def report(self, seconds: float, steps: int) -> dict:
        rep = super().report(seconds, steps)
        rep["gkeys_per_s"] = self.ctx.world * (self.a.numel() + self.b.numel()) * steps / seconds / 1e9
        rep["kept"] = int(self.out[-1].item())
        return rep

    def check(self, reduce: bool = True):
        """The outputs of the timed step against reference(), exactly: the count, the kept keys bit for bit, and the
        indices or the payload (which names every element's place in the concatenation). Local only."""
        ref = self.reference()
        k = int(self.out[-1].item())
        cat = torch.cat([self.a, self.b]).view(torch.int32)
        ok = k == ref.numel() and torch.equal(self.out[0][:k].view(torch.int32), cat[ref])
        if ok and self.mode != "keys":
            ok = self.out[1].dtype == torch.int32 and torch.equal(self.out[1][:k], ref.int())
        ok = bool(ok)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"elements_checked": self.a.numel() + self.b.numel(), "kept": k, "exact_vs_torch": ok, "check_passed": ok}


class SpMM(Workload):
    """Y = A X for a CSR matrix and a dense block of k vectors per GPU (csrc/kernels/spmm.hip, ops.spmm). matrix
    "powerlaw" (ops.powerlaw_csr(n_rows, nnz)), "banded" (the reference's 5-band geometry 401 200 100 200 10 on n_rows
    rows; nnz follows) or "uniform" (every row round(nnz / n_rows) nonzeros in uniformly drawn columns). item_nnz: the
    plan's item size (None: ops.spmm's default for k). GFLOP/s = 2 nnz k / time. No communication (weak scaling).
    csr: a prebuilt matrix to use instead."""

    MATRICES = ("powerlaw", "banded", "uniform")
    BAND = (401, 200, 100, 200, 10)
    SAMPLE = 2048  # rows the check compares with fp64

    def __init__(self, ctx, n_rows=1_000_000, nnz=10_000_000, k=64, matrix="powerlaw", item_nnz=None, csr=None, **_):
        n_rows, nnz, k = int(n_rows), int(nnz), int(k)
        if matrix not in self.MATRICES:
            raise ValueError(f"spmm matrix {matrix!r}: one of {self.MATRICES}")
        if n_rows < 1 or k < 1 or nnz < 0:
            raise ValueError(f"spmm n_rows = {n_rows}, nnz = {nnz}, k = {k}: at least one row and column, nnz >= 0")
        if csr is not None:  # a prebuilt ops.CSR (scripts/spmm_lab.py shares one matrix between its cases)
            m, n_rows = csr, csr.n_rows
        elif matrix == "powerlaw":
            m = ops.powerlaw_csr(n_rows, nnz, seed=1 + ctx.rank)
        elif matrix == "banded":
            if n_rows < 2048:
                raise ValueError("spmm matrix 'banded': at least 2048 rows (the bands reach 710 columns)")
            m = ops.banded_csr(n_rows, *self.BAND)
        else:
            g = torch.Generator().manual_seed(25000 + ctx.rank)
            per_row = max(1, round(nnz / n_rows))
            rp = torch.arange(n_rows + 1, dtype=torch.int64) * per_row
            col = torch.randint(0, n_rows, (n_rows * per_row,), generator=g, dtype=torch.int32)
            m = ops.CSR(rp, col, torch.rand(n_rows * per_row, generator=g) * 2 - 1, n_rows)
        self.item_nnz = ops.sparse.spmm_item_nnz(k) if item_nnz is None else int(item_nnz)
        super().__init__(ctx, {"n_rows": n_rows, "nnz": m.nnz, "k": k, "matrix": matrix, "item_nnz": self.item_nnz},
                         "spmm", "GFLOP/s")
        self.m = m if m.val.device == torch.device(ctx.device) else m.to(ctx.device)
        g = torch.Generator(device=ctx.device).manual_seed(25100 + ctx.rank)
        self.x = torch.rand(m.n_cols, k, device=ctx.device, generator=g) * 2 - 1
        self.out = torch.empty(n_rows, k, device=ctx.device)
        if self.x.is_cuda:
            self.m.spmm_plan(self.item_nnz)  # the host analysis, once per matrix: outside the timed steps

    def step(self):
        ops.spmm(self.m, self.x, out=self.out, item_nnz=self.item_nnz)

    def work_per_step(self):
        return 2.0 * self.m.nnz * self.x.shape[1]

    def compulsory_bytes(self) -> int:
        """col and val read once, X read once, Y written once."""
        return 8 * self.m.nnz + 4 * self.x.shape[1] * (self.m.n_cols + self.m.n_rows)

    def check(self, reduce: bool = True):
        """A fixed seeded sample of rows (with the first, the last and the longest row) against the fp64 product: every
        entry within the any-order bound len u / (1 - len u) * sum|v x| (u = 2^-24; one rounding per product and per
        addition, whatever the order), an empty row exactly 0. Local only."""
        m, k = self.m, self.x.shape[1]
        lens = m.row_ptr[1:] - m.row_ptr[:-1]
        g = torch.Generator().manual_seed(25200)
        rows = torch.randint(0, m.n_rows, (min(self.SAMPLE, m.n_rows),), generator=g)
        rows = torch.unique(torch.cat([rows, torch.tensor([0, m.n_rows - 1, int(lens.argmax())])])).to(lens.device)
        ln = lens[rows]
        seg = torch.repeat_interleave(torch.arange(rows.numel(), device=ln.device), ln)
        nz = torch.arange(seg.numel(), device=ln.device) - (ln.cumsum(0) - ln)[seg] + m.row_ptr[rows][seg]
        v, c = m.val[nz].double()[:, None], m.col[nz].long()
        worst, ok = 0.0, True
        ku = (ln.double() * 2.0 ** -24)[:, None]
        for c0 in range(0, k, 32):
            prod = v * self.x[c, c0:c0 + 32].double()
            ref = torch.zeros(rows.numel(), prod.shape[1], dtype=torch.float64, device=prod.device).index_add_(0, seg, prod)
            bound = ku / (1 - ku) * torch.zeros_like(ref).index_add_(0, seg, prod.abs())
            err = (self.out[rows, c0:c0 + 32].double() - ref).abs()
            ok = ok and bool((err <= bound).all())
            worst = max(worst, float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0)
        if reduce:
            ok = self.ctx.max_over_ranks(0.0 if ok else 1.0) == 0.0
        return {"rows_checked": int(rows.numel()), "worst_err_over_bound": worst, "check_passed": bool(ok)}

    def report(self, seconds: float, steps: int) -> dict:
        rep = super().report(seconds, steps)
        rep["compulsory_gb_per_s"] = self.ctx.world * self.compulsory_bytes() * steps / seconds / 1e9
        rep["gathered_gb_per_s"] = self.ctx.world * 4.0 * self.m.nnz * self.x.shape[1] * steps / seconds / 1e9
        return rep


WORKLOADS = {"sgemm": Sgemm, "reduce": Reduce, "scan": Scan, "stencil": Stencil, "spmv": SpMV, "spmm": SpMM,
             "region3d": Region3D, "raycast": Raycast, "histeq": Histeq, "region2d": Region2D, "select": Select,
             "sort": Sort, "segreduce": SegReduce, "topk": TopK, "scanbykey": ScanByKey, "bincount": Bincount,
             "merge": Merge, "rowsort": RowSort, "axis": Axis, "ragged": Ragged, "segsort": SegSort,
             "argreduce": ArgReduce, "setops": SetOps}


def build_workload(name: str, ctx: Context, **cfg) -> Workload:
    return WORKLOADS[name](ctx, **cfg)
