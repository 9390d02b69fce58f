"""The oracle of the set operations on sorted sequences (ops.set_* / csrc/kernels/setops.hip), written from the
definition with torch ops so that it runs on either device, a brute-force per-key counter in plain Python that shares
no code with it, and the input families of the set-op tests. No GPU is needed to import or to run this module.

Definition. Two elements are equal when their transformed keys (key64: radix_key.h's to_key) are equal. A key occurs
m times in a and n times in b; the i-th occurrence in a is PAIRED with the i-th in b for i < min(m, n).
    intersection          the paired elements of a
    union                 all of a and the unpaired elements of b
    difference            the unpaired elements of a
    symmetric_difference  the unpaired elements of both
The result is the kept elements in the order of the stable sort of cat(a, b) (a tie goes to a), given as int32
positions in the concatenation and the concatenation's bits gathered with them.

set_oracle takes `mutant`: one of MUTANTS turns on a single fault, which the CPU tests must be able to tell from the
brute force (tests/test_setops_cpu.py::test_assertions_reject_mutants)."""
import torch

T = 4352  # csrc/kernels/setops.hip kTile: merged positions per block
OPS = ["intersection", "union", "difference", "symmetric_difference"]
DTYPES = [torch.float32, torch.int32]
KINDS = ["ties", "a_below_b", "a_above_b", "interleaved", "all_equal", "specials"]
SMALL = [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 7]
SIZE_PAIRS = [(na, nb) for na in SMALL for nb in SMALL] + [(257 * T + 13, 3), (3, 257 * T + 13), (129 * T + 5, 128 * T + 9)]
RUN_LENGTHS = [1, 3, T - 1, T, T + 1, 3 * T]
F32_SPECIAL_BITS = [0xff800000, 0xc0000000, 0x80000001, 0x80000000, 0x00000000, 0x00000001, 0x3f800000, 0x7f800000,
                    0x7fc00000, 0xffc12345, 0x7f800001, 0x7fffffff, 0xffffffff]
I32_EXTREMES = [-2**31, -2**31 + 1, -1, 0, 1, 2**31 - 2, 2**31 - 1]
MUTANTS = ["first_unpaired", "tie_to_b", "no_carry_in", "no_carry_out", "set_counting", "bits_from_b"]


def capacity(op, na, nb):
    return {"intersection": min(na, nb), "difference": na}.get(op, na + nb)


def bits(t):
    return t.view(torch.int32)


def key64(x, descending):
    """radix_key.h to_key with torch ops: int64 keys whose ascending order is the ops' order"""
    b = bits(x.reshape(-1).contiguous()).long() & 0xFFFFFFFF
    if x.dtype == torch.float32:
        mag = b & 0x7FFFFFFF
        k = torch.where(b >= 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)
        k = torch.where(mag == 0, torch.full_like(k, 0x80000000), k)
        k = torch.where(mag > 0x7F800000, torch.full_like(k, 0xFFFFFFFF), k)
    else:
        k = b ^ 0x80000000
    return 0xFFFFFFFF - k if descending else k


def sort_by_key64(x, descending):
    """flat x sorted in the ops' order by the stable sort of its int64 keys (right for NaNs of either sign on both
    devices: see the docstring of tests/test_gpu_merge.py), every element's bits kept"""
    return bits(x.reshape(-1))[torch.sort(key64(x, descending), stable=True).indices].view(x.dtype)


def specials(dtype, dev):
    if dtype == torch.float32:
        return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in F32_SPECIAL_BITS], dtype=torch.int32,
                            device=dev).view(torch.float32)
    return torch.tensor(I32_EXTREMES, dtype=torch.int32, device=dev)


def side(kind, which, n, dtype, descending, gen, dev):
    """n sorted keys of side `which` (0 = a, 1 = b); the families of the merge tests"""
    if kind == "ties":
        x = torch.randint(0, 8, (n,), device=dev, generator=gen)
    elif kind in ("a_below_b", "a_above_b"):
        low = (which == 0) == (kind == "a_below_b")
        x = torch.randint(0, 100, (n,), device=dev, generator=gen) + (0 if low else 100)
    elif kind == "interleaved":
        x = 2 * torch.arange(n, device=dev) + which
    elif kind == "all_equal":
        x = torch.full((n,), 5, device=dev)
    elif kind == "specials":
        sp = specials(dtype, dev)
        x = sp[torch.randint(0, sp.numel(), (n,), device=dev, generator=gen)]
    else:
        raise ValueError(kind)
    return sort_by_key64(x.to(dtype), descending)


def runs_side(n, length, dtype, descending, dev):
    """the `runs` family: key i // length"""
    return sort_by_key64(torch.div(torch.arange(n, device=dev), length, rounding_mode="floor").to(dtype), descending)


def _counts(k_self, k_other):
    """per element of sorted k_self: its rank in its run, the run's length, and the length of k_other's run of its key"""
    i = torch.arange(k_self.numel(), device=k_self.device)
    rank = i - torch.searchsorted(k_self, k_self, right=False)
    own = torch.searchsorted(k_self, k_self, right=True) - torch.searchsorted(k_self, k_self, right=False)
    other = torch.searchsorted(k_other, k_self, right=True) - torch.searchsorted(k_other, k_self, right=False)
    return rank, own, other


def set_oracle(a, b, op, descending=False, mutant=None, tile=T):
    """(int32 bits of the kept elements, their int32 positions in cat(a.flatten(), b.flatten())) in merge order"""
    return set_oracle_all(a, b, descending, mutant, tile, only=(op,))[op]


def set_oracle_all(a, b, descending=False, mutant=None, tile=T, only=OPS):
    """{op: set_oracle(a, b, op)} with the order and the pairing computed once"""
    af, bf = a.reshape(-1), b.reshape(-1)
    na, nb = af.numel(), bf.numel()
    dev = af.device
    ka, kb = key64(af, descending), key64(bf, descending)
    if mutant == "tie_to_b":  # the stable sort of b ++ a, mapped back to positions in a ++ b
        o = torch.sort(torch.cat([kb, ka]), stable=True).indices
        order = torch.where(o < nb, o + na, o - nb)
    else:
        order = torch.sort(torch.cat([ka, kb]), stable=True).indices
    rank_a, m_a, n_b = _counts(ka, kb)
    rank_b, n_own, m_of_b = _counts(kb, ka)
    if mutant in ("no_carry_in", "no_carry_out"):
        # what a tile of `tile` merged positions sees when the counts that cross its borders are dropped. Inside a
        # run the merged order is the m elements of a, then the n of b.
        pos = torch.empty(na + nb, dtype=torch.long, device=dev)
        pos[order] = torch.arange(na + nb, device=dev)
        pa, pb = pos[:na], pos[na:]
        if mutant == "no_carry_in":  # ranks restart at the tile's first position
            rank_a = pa - torch.maximum(pa - rank_a, pa // tile * tile)
            rank_b = pb - torch.maximum(pb - rank_b, pb // tile * tile)
        else:                        # partners behind the tile's last position are not counted
            first_b = pa - rank_a + m_a
            n_b = (torch.minimum(first_b + n_b, (pa // tile + 1) * tile) - first_b).clamp(min=0)
    if mutant == "set_counting":
        paired_a, paired_b = n_b > 0, m_of_b > 0
    elif mutant == "first_unpaired":  # pairs the LAST min(m, n) of each run, so the first ones are left over
        paired_a, paired_b = m_a - 1 - rank_a < n_b, n_own - 1 - rank_b < m_of_b
    else:
        paired_a, paired_b = rank_a < n_b, rank_b < m_of_b
    masks = {"intersection": (paired_a, torch.zeros_like(paired_b)),
             "union": (torch.ones_like(paired_a), ~paired_b),
             "difference": (~paired_a, torch.zeros_like(paired_b)),
             "symmetric_difference": (~paired_a, ~paired_b)}
    cat_bits, out = bits(torch.cat([af, bf])), {}
    for op in only:
        idx = order[torch.cat(masks[op])[order]]
        if mutant == "bits_from_b" and op == "intersection":  # the partner in b instead of the element of a
            idx = na + torch.searchsorted(kb, ka[idx], right=False) + rank_a[idx]
        out[op] = (cat_bits[idx], idx.int())
    return out


def brute_force(a, b, op, descending=False):
    """The positions in cat(a, b) of the result, as a Python list, from a per-key count: no searchsorted, no sort of
    the concatenation. For small inputs."""
    ka, kb = key64(a, descending).tolist(), key64(b, descending).tolist()
    na = len(ka)
    where_a, where_b = {}, {}
    for i, k in enumerate(ka):
        where_a.setdefault(k, []).append(i)
    for j, k in enumerate(kb):
        where_b.setdefault(k, []).append(na + j)
    out = []
    for k in sorted(set(where_a) | set(where_b)):
        ia, ib = where_a.get(k, []), where_b.get(k, [])
        p = min(len(ia), len(ib))
        if op == "intersection":
            out += ia[:p]
        elif op == "union":
            out += ia + ib[p:]
        elif op == "difference":
            out += ia[p:]
        else:
            out += ia[p:] + ib[p:]
    return out
