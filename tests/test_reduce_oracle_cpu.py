"""The oracle of the device-wide reduce / dot / scan tests, checked on the CPU: the index model of reduce.hip takes
every element and every partial exactly once at every size where its shape changes, the exact families are exact in
any order, the derived bounds hold for a float32 emulation in the kernel's order, and every single-fault mutant of the
model is rejected by the assertion functions the GPU tests use (tests/_reduce_oracle.py)."""
import numpy as np
import pytest
import torch

import _reduce_oracle as ro

CAPS = (1, 2, 3, 7, ro.CAP)


@pytest.mark.parametrize("cap", CAPS)
def test_coverage_takes_every_element_and_partial_once(cap):
    seen_np_tail, seen_np = set(), set()
    for n in ro.interesting_n(cap):
        c = ro.coverage(n, cap)
        assert c.exactly_once, (n, cap, np.nonzero(c.elem_count != 1)[0][:8], np.nonzero(c.part_count != 1)[0][:8])
        assert c.nb == ro.pass1_blocks(n, cap) <= cap
        seen_np_tail.add(c.np_tail)
        seen_np.add(c.nb)
    if cap == ro.CAP:
        assert seen_np >= set(range(1, 10)) and seen_np_tail == {0, 1, 2, 3}
    else:
        assert seen_np == set(range(1, cap + 1))


def test_interesting_sizes_reach_every_loop_region():
    """What the GPU tests assert about the sizes they run, from `coverage`: trips >= 2 and >= 3 on the capped grids,
    a second trip that is partly clean-up, clean-up and tail taken, np & 3 in all four states, live pass-2 fill."""
    for cap in (1, 3, 7):
        cs = [ro.coverage(n, cap) for n in ro.interesting_n(cap)]
        assert max(c.trips for c in cs) >= 3 and any(c.trips == 2 for c in cs)
        assert any(("cleanup", 1) in c.regions and ("unrolled", 1) in c.regions for c in cs)
        assert any(("cleanup", 2) in c.regions for c in cs)
        assert {c.n & 3 for c in cs} == {0, 1, 2, 3}
    cs = [ro.coverage(n) for n in ro.interesting_n()]
    assert all(c.trips == 1 for c in cs) and {c.np_tail for c in cs} == {0, 1, 2, 3}
    assert any(c.fill_live > 0 for c in cs) and any(c.cleanup_taken for c in cs)
    assert max(ro.interesting_n(7)) < 400_000


def test_coverage_of_the_production_grid_above_its_cap():
    """2^26 + 4096 * 5 + 3 on 16384 blocks: arithmetic only. Five blocks take a second unrolled trip; the second size
    adds a sixth block that is partly in the clean-up loop."""
    c = ro.coverage_counts(ro.BIG_N[0])
    assert c.exactly_once and c.nb == ro.CAP and c.trips == 2
    assert c.regions == {("unrolled", 0): 1 << 24, ("unrolled", 1): 5 * ro.CHUNK} and c.depth == 17
    c = ro.coverage_counts(ro.BIG_N[1])
    assert c.exactly_once and c.trips == 2 and c.regions[("cleanup", 1)] > 0 and c.regions[("unrolled", 1)] > 5 * ro.CHUNK
    small = ro.coverage_counts(86023, 7, batch=2)  # the batched walk agrees with the table walk
    full = ro.coverage(86023, 7)
    assert small.exactly_once and small.depth == full.depth and small.trips == full.trips == 4


def test_probe_positions_name_every_region():
    for n, cap in ro.PROBE_CASES:
        cap = ro.CAP if cap is None else cap
        c, pos = ro.coverage(n, cap), ro.probe_positions(n, cap)
        assert 0 < len(pos) <= 72 and set(range(c.n4 * 4, n)) <= set(pos)
        vec = np.array([p >> 2 for p in pos if p < c.n4 * 4])
        hit = set(zip(c.vec_region[vec].tolist(), c.vec_trip[vec].tolist(), c.vec_slot[vec].tolist()))
        every = set(zip(c.vec_region.tolist(), c.vec_trip.tolist(), c.vec_slot.tolist()))
        assert hit == every, every - hit


@pytest.mark.parametrize("cap", (3, ro.CAP))
def test_exact_and_weighted_families_are_exact_in_any_order(cap):
    """float32 sums in the model's order and in two scrambled sequential orders give the int64 truth."""
    run = ro.model_run()
    for n in ro.interesting_n(cap):
        ro.check_exact_size(run, n, cap)
    for family in (ro.exact_family, ro.weighted_family):
        for n in ro.interesting_n(cap)[::9]:
            x, total = family(n)
            for seed in (1, 2):
                perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
                assert float(np.cumsum(x[perm].numpy(), dtype=np.float32)[-1]) == total, (n, seed)


def test_model_passes_the_gpu_assertions():
    assert ro.rejecting_checks(ro.model_run()) == set()


def test_dense_bound_holds_for_the_model():
    worst = 0.0
    for n, cap in ((4 * 900 + 3, ro.CAP), (100_003, ro.CAP), (1 << 18, ro.CAP), (86023, 7), (36871, 3), (34839, 1)):
        x, ref, mag = ro.dense_family(n)
        got = float(ro.emulate("sum", x, None, cap))
        bound = ro.sum_bound(ro.depth(n, cap), mag, ref)
        assert abs(got - ref) <= bound, (n, cap)
        worst = max(worst, abs(got - ref) / bound)
        y, _, _ = ro.dense_family(n, seed=9)
        ref = float((x.double() * y.double()).sum())
        got = float(ro.emulate("sum", x, y, cap))
        assert abs(got - ref) <= ro.sum_bound(ro.depth(n, cap, prod=True), float((x.double() * y.double()).abs().sum()), ref)
    assert 0.0 < worst < 1.0


@pytest.mark.parametrize("n", [5000, ro.TILE * 2 + 3])
@pytest.mark.parametrize("exclusive", [False, True])
def test_scan_bound_and_exactness_hold_for_the_model(n, exclusive):
    x, _, _ = ro.dense_family(n, seed=4)
    ref = torch.cumsum(x.double(), 0).numpy()
    bound = ro.scan_bound(x)
    if exclusive:
        ref, bound = np.concatenate([[0.0], ref[:-1]]), np.concatenate([[0.0], bound[:-1]])
    err = np.abs(ro.emulate_scan(x, exclusive).astype(np.float64) - ref)
    assert (err <= bound).all() and err.max() > 0
    for family in (ro.scan_exact_family, ro.scan_weighted_family):
        xe, refe = family(n)
        want = ro.scan_truth(refe, exclusive, 3.0).numpy()
        assert np.array_equal(ro.emulate_scan(xe, exclusive, 3.0), want)


def test_scan_depth_grows_by_tile_and_position():
    d = ro.scan_depth(np.arange(ro.TILE * 3), ro.TILE * 3)
    assert d[0] == 3 + 6 + 0 + 4 and d[ro.TILE - 1] == 3 + 6 + 16 + 1 + 7 + 3
    assert d[ro.TILE] == 3 + 6 + 16 + 8 + 8 + 2 and d[2 * ro.TILE] == d[ro.TILE] + 8
    assert (np.diff(d.reshape(3, -1).max(1)) > 0).all()


# the assertion group that has to reject each mutant (more may)
MUTANTS = {
    "tail_every_block": "exact", "tail_dropped": "exact", "dot_tail_xx": "exact", "cleanup_short": "exact",
    "no_second_trip": "exact", "stride_off": "exact", "slot3_reads_slot2": "exact", "pass2_tail_dropped": "exact",
    "pass2_fill_zero": "probes", "dot_y_from_x": "exact", "sum_identity_negzero": "specials",
    "min_hands_on_nan": "specials", "minmax_tree": "specials",
}


def test_mutant_list_is_the_oracles():
    assert set(MUTANTS) == set(ro.FAULTS) and len(MUTANTS) >= 12


@pytest.mark.parametrize("fault", sorted(MUTANTS))
def test_mutant_is_rejected(fault):
    rejected = ro.rejecting_checks(ro.model_run(fault), only=(MUTANTS[fault],))
    assert MUTANTS[fault] in rejected, (fault, rejected)
    if fault in ("tail_every_block", "tail_dropped", "cleanup_short", "no_second_trip", "stride_off",
                 "slot3_reads_slot2", "pass2_tail_dropped"):  # coverage itself sees the faults in who takes what
        caps = [ro.CAP, 1, 3, 7]
        assert any(not ro.coverage(n, cap, fault=fault).exactly_once for cap in caps for n in ro.interesting_n(cap))


def test_mutants_are_caught_by_the_probes_too():
    """A position names the loop region: the index faults are also rejected by the planted-element checks alone."""
    for fault in ("tail_dropped", "cleanup_short", "no_second_trip", "stride_off", "slot3_reads_slot2", "dot_y_from_x",
                  "dot_tail_xx", "tail_every_block"):
        with pytest.raises(AssertionError):
            for n, cap in ro.PROBE_CASES:
                ro.check_probes(ro.model_run(fault), n, cap)
