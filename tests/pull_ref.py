"""Plain numpy restatement of what the mailbox's two all-reduces promise (include/mtd_abi.h: mtd_comm_allreduce_small,
mtd_comm_allreduce_pull; comm.hip), the inputs the GPU tests feed them and the lengths they run at.

The promise is a sum "added up in rank order … the same bits on every rank": `rank_order_sum` is that sum, IEEE double additions
one after the other starting from +0.0, so the GPU comparison (tests/test_gpu_comm_pull.py) is on BITS and carries no tolerance.
tests/test_pull_ref.py checks this file: that `slices` is a partition, that `COUNTS` reaches every kind of slice layout, and that
the generated inputs make a wrong summation order visible.
"""
import numpy as np

STRIDE = 2048 * 256                 # elements one sweep of a pull launch covers (comm.hip: at most 2048 blocks of 256 threads)
CAP = 2 * STRIDE + 65               # attached capacity of the GPU tests: at two ranks ONE SLICE exceeds a sweep (the reduce launch wraps)
SENTINELS = 64                      # doubles behind `count` in every device buffer that no kernel may touch

# fixed places of the planted specials (each is planted where it lies below `count`)
I_NEG_ZERO, I_DENORMAL, I_INF, I_INF_PAIR, I_NAN, I_CANCEL = 0, 3, 5, 7, 11, 13


def rank_order_sum(xs):
    """elementwise +0.0 + xs[0] + xs[1] + …, one rounding per addition, in float64"""
    acc = np.zeros(len(xs[0]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for x in xs:
            acc = acc + np.asarray(x, dtype=np.float64)
    return acc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def chunk(count, world):
    """doubles per slice: count / world rounded up, then up to a multiple of 32"""
    per_rank = -(-count // world)
    return -(-per_rank // 32) * 32


def slices(count, world):
    """[lo, hi) of the slice rank r reduces, r = 0 … world-1: rank r owns [r·chunk, min((r+1)·chunk, count)) — empty where
    r·chunk >= count (returned as lo == hi == count)"""
    c = chunk(count, world)
    return [(min(r * c, count), min((r + 1) * c, count)) for r in range(world)]


def inputs(count, rank, seed, world):
    """rank `rank`'s contribution to an all-reduce of `count` doubles over `world` ranks: normal deviates scaled by
    2**randint(-30, 30) — neighbouring ranks' values rarely share an exponent, so the order of the additions shows in the last
    bits — with specials planted at fixed indices.  Every rank can compute every rank's array."""
    rng = np.random.default_rng([int(seed), int(count), int(world), int(rank)])
    x = np.ldexp(rng.standard_normal(count), rng.integers(-30, 31, count, dtype=np.int32))
    last = world - 1

    def plant(i, v):
        if i < count:
            x[i] = v

    plant(I_NEG_ZERO, -0.0)                                     # on every rank: the sum starts from +0.0, so it is +0.0
    plant(I_DENORMAL, (rank + 1) * 5e-324)                      # denormal operands and a denormal sum
    if rank == last:
        plant(I_INF, np.inf)                                    # +inf on one rank
    if rank == 0:
        plant(I_INF_PAIR, np.inf)                               # +inf and -inf at one index: NaN
    elif rank == 1:
        plant(I_INF_PAIR, -np.inf)
    if rank == 1 % world:
        plant(I_NAN, np.nan)                                    # an arithmetic NaN on one rank
    big = float(np.random.default_rng([int(seed), int(count), int(world)]).standard_normal()) * 2.0 ** 40 + 2.0 ** 41
    if rank == 0:
        plant(I_CANCEL, big)                                    # cancels against the last rank's; what the ranks between
    elif rank == last:                                          # add survives only in part, depending on the order
        plant(I_CANCEL, -big)
    return x


def sentinels():
    """the doubles placed behind `count`: finite, each different, nothing a sum of the inputs produces"""
    return -1.25e300 - np.arange(SENTINELS, dtype=np.float64) * 1e285


def COUNTS(world, cap=CAP):
    """the lengths of the GPU test at `world` ranks and capacity `cap`"""
    raw = [1, 31, 32, 33, 32 * world - 1, 32 * world, 32 * world + 1, STRIDE + 77, cap - 1, cap]
    out = []
    for c in raw:
        if 1 <= c <= cap and c not in out:
            out.append(c)
    return out


def back_to_back(world, cap=CAP):
    """the lengths of one round of the back-to-back scenario"""
    return [cap, 1, 33, cap - 1, 32 * world, 7]


def small_max(world):
    """the largest small all-reduce whose image in the kernel's local memory fits (8·n·world <= 60000 bytes)"""
    return 60000 // (8 * world)


def compare(got, want):
    """what the GPU tests assert about one result (arrays of equal length): number of elements whose bits differ where the
    expectation is not NaN, number of elements whose NaN-ness differs, and the first few offending indices"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan_w, nan_g = np.isnan(want), np.isnan(got)
    bad_bits = (~nan_w) & (bits(got) != bits(want))
    bad_nan = nan_w != nan_g
    where = np.flatnonzero(bad_bits | bad_nan)
    return dict(bad_bits=int(bad_bits.sum()), bad_nan=int(bad_nan.sum()), first_bad=[int(i) for i in where[:4]])


# seeds: scenario base + call number
SEED_COUNTS, SEED_ROUNDS, SEED_SMALL, SEED_REFUSED, SEED_CAP, SEED_TIMEOUT = 1000, 2000, 3000, 4000, 5000, 6000
