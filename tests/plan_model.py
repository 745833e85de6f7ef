"""A host model of the single-frame planner (atray_amd/csrc/plan.hip): the block
list a plan writes, restated in plain Python/numpy from the kernels' code and comments. Exact, not
statistical: given the costs and the thresholds carried over from the previous plan the kernels
are deterministic, so tests/test_gpu_plan.py compares whole lists byte for byte.

A block is the 32-byte DBlock of engine.h (DBLOCK). A plan of nb base blocks writes nb + max_split
blocks: the base blocks graded into 8 classes by the cost bucket of their cell (class 0 first, base
order inside a class), the heaviest split into two or four row-band waves on consecutive slots,
the rest of the list empty blocks. The thresholds that grade and split lag one plan behind the
costs: plan n orders by the thresholds derived from plan n - 1's histogram (PlanState)."""
import numpy as np

DBLOCK = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("mask_lo", "<u4"), ("mask_hi", "<u4"),
                   ("out_base", "<i4"), ("flags", "<i4"), ("base", "<i4"), ("pad", "<i4")])
assert DBLOCK.itemsize == 32

BUCKETS = 256  # 8 per power of two of the clock count
CLASSES = 8
# cumulative fractions of the cells, heaviest first, that end classes 0..6 (f32, as kClassFrac)
CLASS_FRAC = tuple(np.float32(f) for f in (0.02, 0.05, 0.10, 0.20, 0.30, 0.50, 0.75))
SPLIT2_DEFAULT, SPLIT4_DEFAULT = 0.01, 0.0  # what a negative split2 / split4 means
BLOCK_PRIO = 1  # kBlockPrio


class Thresholds:
    """thr[k]: bucket >= thr[k] (first such k) -> class k; bucket >= split4_thr: four waves,
    >= split_thr: two. All zero (the work area before its first plan): one class, no split."""

    def __init__(self, thr=(0,) * CLASSES, split_thr=0, split4_thr=0):
        self.thr = tuple(int(t) for t in thr)
        self.split_thr, self.split4_thr = int(split_thr), int(split4_thr)
        assert len(self.thr) == CLASSES

    def __eq__(self, o):
        return (self.thr, self.split_thr, self.split4_thr) == (o.thr, o.split_thr, o.split4_thr)

    def __repr__(self):
        return f"Thresholds({self.thr}, split_thr={self.split_thr}, split4_thr={self.split4_thr})"


def cost_bucket(c):
    """floor(log2 c) * 8 + the next three bits below the leading one, clamped to 255; 0 -> 0."""
    c = int(c)
    assert 0 <= c < 1 << 64
    if c == 0:
        return 0
    e = c.bit_length() - 1
    m = (c >> (e - 3)) & 7 if e >= 3 else (c << (3 - e)) & 7
    return min(e * 8 + m, BUCKETS - 1)


def cost_buckets(cost):
    """cost_bucket of every element of a u64 array."""
    c = np.asarray(cost, np.uint64)
    e = np.zeros(c.shape, np.int64)
    t = c.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = (t >> np.uint64(s)) != 0
        e += big * s
        t = np.where(big, t >> np.uint64(s), t)
    down = (c >> np.maximum(e - 3, 0).astype(np.uint64)) & np.uint64(7)
    up = (c << np.maximum(3 - e, 0).astype(np.uint64)) & np.uint64(7)
    b = e * 8 + np.where(e >= 3, down, up).astype(np.int64)
    return np.where(c == 0, 0, np.minimum(b, BUCKETS - 1))


def block_class(T, bucket):
    k = 0
    while k < CLASSES - 1 and bucket < T.thr[k]:
        k += 1
    return k


def block_parts(T, bucket):
    if T.split_thr == 0:
        return 1
    return 4 if bucket >= T.split4_thr else (2 if bucket >= T.split_thr else 1)


def next_thresholds(hist, nb, max_split, split2=-1.0, split4=-1.0):
    """The thresholds the next plan orders by, from this plan's histogram. The cells above a bucket
    decide its class (the class fractions they reach); whole buckets from the top split while they
    fit the fraction (+ half a cell) and the spare capacity, four ways first. The comparisons are
    the kernel's, in f32 with the multiply and the add rounded separately."""
    f32 = np.float32
    split2 = f32(SPLIT2_DEFAULT if split2 < 0 else split2)
    split4 = f32(SPLIT4_DEFAULT if split4 < 0 else split4)
    hist = [int(h) for h in hist]
    assert len(hist) == BUCKETS
    fnb = f32(nb)
    lim2 = f32(f32(split2 * fnb) + f32(0.5))
    lim4 = f32(f32(split4 * fnb) + f32(0.5))
    incl = [0] * BUCKETS
    s = 0
    for b in range(BUCKETS - 1, -1, -1):
        s += hist[b]
        incl[b] = s
    s4 = [hist[b] > 0 and f32(incl[b]) <= lim4 and 3 * incl[b] <= max_split for b in range(BUCKETS)]
    n4 = max([incl[b] for b in range(BUCKETS) if s4[b]], default=0)  # cells taking four waves
    s2 = [hist[b] > 0 and not s4[b] and f32(incl[b]) <= lim2 and 3 * n4 + (incl[b] - n4) <= max_split
          for b in range(BUCKETS)]
    thr = [BUCKETS] * CLASSES
    for b in range(BUCKETS):
        if not hist[b]:
            continue
        above = f32(incl[b] - hist[b])
        k = 0
        while k < CLASSES - 1 and above >= f32(CLASS_FRAC[k] * fnb):
            k += 1
        thr[k] = min(thr[k], b)
    last = BUCKETS
    for j in range(CLASSES):  # a class with no bucket takes the previous class's threshold
        if thr[j] == BUCKETS:
            thr[j] = last
        last = thr[j]
    thr[CLASSES - 1] = 0  # everything else is the last class
    split_thr = min([b for b in range(BUCKETS) if s2[b] or s4[b]], default=BUCKETS)
    split4_thr = min([b for b in range(BUCKETS) if s4[b]], default=BUCKETS)
    # 0 marks "before the first plan": a derived 0 becomes 1
    return Thresholds(thr, split_thr if split_thr > 0 else 1, split4_thr if split4_thr > 0 else 1)


def _popcount(m):
    return np.unpackbits(np.ascontiguousarray(m, np.uint64).view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def plan(base_blocks, cost, T_use, max_split):
    """The list of one plan under the thresholds T_use: (nb + max_split DBLOCKs, used, nosplit)."""
    base_blocks = np.asarray(base_blocks, DBLOCK)
    nb = base_blocks.size
    cap = nb + int(max_split)
    bkt = cost_buckets(cost)
    assert bkt.shape == (nb,)
    below = np.ones(nb, bool)  # block_class: the first k with bucket >= thr[k]
    k = np.zeros(nb, np.int64)
    for j in range(CLASSES - 1):
        below &= bkt < T_use.thr[j]
        k += below
    if T_use.split_thr == 0:
        parts = np.ones(nb, np.int64)
    else:
        parts = np.where(bkt >= T_use.split4_thr, 4, np.where(bkt >= T_use.split_thr, 2, 1))
    # the carried-over split thresholds may select more cells than the list has room for: no splits
    nosplit = int(parts.sum() > cap)
    if nosplit:
        parts = np.ones(nb, np.int64)
    used = int(parts.sum())
    order = np.argsort(k, kind="stable")  # classes 0..7, base order inside a class
    slot = np.empty(nb, np.int64)
    slot[order] = np.cumsum(parts[order]) - parts[order]
    out = np.zeros(cap, DBLOCK)  # the tail: empty blocks
    m = base_blocks["mask_lo"].astype(np.uint64) | (base_blocks["mask_hi"].astype(np.uint64) << np.uint64(32))
    for p in range(4):
        sel = np.flatnonzero(parts > p)
        if sel.size == 0:
            break
        bits = (64 // parts[sel]).astype(np.uint64)  # 8 pixels per row, 8 / parts rows per band
        lo = bits * np.uint64(p)  # < 64 whenever parts > 1
        band = np.where(parts[sel] == 1, ~np.uint64(0), ((np.uint64(1) << (bits % np.uint64(64))) - np.uint64(1)) << lo)
        earlier = (np.uint64(1) << lo) - np.uint64(1)
        t = base_blocks[sel].copy()  # x0, y0, flags, base and pad as they are
        t["mask_lo"] = ((m[sel] & band) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        t["mask_hi"] = ((m[sel] & band) >> np.uint64(32)).astype(np.uint32)
        t["out_base"] = base_blocks["out_base"][sel] + _popcount(m[sel] & earlier).astype(np.int32)
        out[slot[sel] + p] = t
    return out, used, nosplit


class PlanState:
    """What a work area carries from plan to plan: `use`, the thresholds the next plan orders by
    (zero before the first). step() is one atr_launch_plan."""

    def __init__(self):
        self.use = Thresholds()

    def step(self, base_blocks, cost, max_split, split2=-1.0, split4=-1.0):
        nb = len(base_blocks)
        out = plan(base_blocks, cost, self.use, max_split)
        hist = np.bincount(cost_buckets(cost), minlength=BUCKETS)
        self.use = next_thresholds(hist, nb, max_split, split2, split4)
        return out


# ---- synthetic inputs, shared by the CPU tests of the model and the GPU tests of the kernels ----
FULL = 0xFFFFFFFF


def bucket_cost(b):
    """The smallest cost in bucket b (b >= 24: from there on every bucket exists)."""
    assert 24 <= b < BUCKETS
    return (8 + b % 8) << (b // 8 - 3)


def distinct_costs(nb):
    """One cell per bucket 24 .. 24 + nb - 1, shuffled; returns (cost, bucket per cell)."""
    b = np.random.default_rng(nb).permutation(np.arange(24, 24 + nb))
    return np.array([bucket_cost(int(x)) for x in b], np.uint64), b


def synthetic_blocks(nb, rng=None):
    """Base blocks with cumulative out_base and base = index: full masks, or (with rng) a mix of
    full, random partial and empty masks and masks of rows 0-3 or 4-7 only (what a user cell plan's
    two-way split leaves), kBlockPrio on some and a pad that must be carried along."""
    a = np.zeros(nb, DBLOCK)
    a["x0"] = 8 * (np.arange(nb) % 61)
    a["y0"] = 8 * (np.arange(nb) // 61)
    a["base"] = np.arange(nb)
    a["mask_lo"] = a["mask_hi"] = FULL
    if rng is not None:
        kind = rng.integers(0, 5, nb)
        lo, hi = rng.integers(0, 1 << 32, nb, dtype=np.uint32), rng.integers(0, 1 << 32, nb, dtype=np.uint32)
        a["mask_lo"] = np.where(kind == 0, np.uint32(FULL), np.where((kind == 1) | (kind == 3), lo, np.uint32(0)))
        a["mask_hi"] = np.where(kind == 0, np.uint32(FULL), np.where((kind == 1) | (kind == 4), hi, np.uint32(0)))
        a["flags"] = rng.integers(0, 2, nb) * BLOCK_PRIO
        a["pad"] = rng.integers(0, 1 << 20, nb)
    m = a["mask_lo"].astype(np.uint64) | (a["mask_hi"].astype(np.uint64) << np.uint64(32))
    pc = np.array([bin(int(x)).count("1") for x in m])
    a["out_base"] = np.cumsum(pc) - pc
    return a


COSTS = {  # name -> (rng, nb) -> u64 clock counts
    "zero": lambda r, n: np.zeros(n, np.uint64),
    "equal": lambda r, n: np.full(n, 4321, np.uint64),
    "two": lambda r, n: np.where(r.random(n) < 0.05, 10**6, 300).astype(np.uint64),
    "lognormal": lambda r, n: np.exp(r.normal(8.0, 1.5, n)).astype(np.uint64),  # as a real frame's
    "heavier": lambda r, n: np.exp(r.normal(10.5, 1.5, n)).astype(np.uint64),
    # 1 .. 2^40: a fifth at or above 2^32, in the clamped top bucket
    "span": lambda r, n: (2.0 ** r.uniform(0, 40, n)).astype(np.uint64),
    # 40 % of the cells tied in one bucket around the median: it straddles the 30 and 50 % fractions
    "ties": lambda r, n: np.where(r.random(n) < 0.4, 5000, np.exp(r.normal(8.5, 2.0, n))).astype(np.uint64),
}
