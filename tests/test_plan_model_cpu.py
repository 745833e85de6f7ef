"""The host model of the single-frame planner (tests/plan_model.py) against hand-worked cases and
properties that do not depend on how the model is written. tests/test_gpu_plan.py holds the
kernels of plan.hip to this model; these tests keep the model from being its own only witness."""
import numpy as np
import pytest

from tests import plan_model as M

FULL = M.FULL
blocks, distinct_costs, COSTS = M.synthetic_blocks, M.distinct_costs, M.COSTS


def mask64(b):
    return int(b["mask_lo"]) | (int(b["mask_hi"]) << 32)


def test_cost_bucket_values():
    want = {0: 0, 1: 0, 2: 8, 3: 12, 7: 22, 8: 24, 9: 25, 15: 31, 16: 32, 2**32 - 1: 255, 2**32: 255, 2**63: 255}
    for c, b in want.items():
        assert M.cost_bucket(c) == b, c
    assert M.cost_buckets(np.array(list(want), np.uint64)).tolist() == list(want.values())
    # 8 buckets per power of two: 2^e (8 + m) / 8 opens bucket 8 e + m, up to the clamp at 2^32
    for e in range(3, 32):
        for m in range(8):
            c = (8 + m) << (e - 3)
            assert M.cost_bucket(c) == 8 * e + m, c
            assert c == 8 or M.cost_bucket(c - 1) == 8 * e + m - 1, c  # below 8, buckets are skipped
    assert M.cost_bucket(2**64 - 1) == 255


def test_cost_buckets_vector_equals_scalar():
    rng = np.random.default_rng(5)
    c = (rng.integers(0, 1 << 63, 4000, dtype=np.uint64) >> rng.integers(0, 64, 4000).astype(np.uint64))
    c = np.concatenate([c, np.array([0, 1, 2, 3, 2**64 - 1], np.uint64)])
    assert M.cost_buckets(c).tolist() == [M.cost_bucket(int(x)) for x in c]


def test_zeroed_thresholds_one_class_one_wave():
    T = M.Thresholds()
    for b in (0, 1, 100, 255):
        assert M.block_class(T, b) == 0 and M.block_parts(T, b) == 1
    base, (cost, _) = blocks(77, np.random.default_rng(1)), distinct_costs(77)
    out, used, nosplit = M.plan(base, cost, T, 9)
    assert (used, nosplit) == (77, 0)
    assert out[:77].tobytes() == base.tobytes() and not out[77:].tobytes().strip(b"\0") and out.size == 86


def test_class_and_parts_lookup():
    T = M.Thresholds((220, 214, 204, 204, 164, 124, 74, 0), split_thr=210, split4_thr=218)
    assert [M.block_class(T, b) for b in (255, 220, 219, 214, 213, 204, 203, 164, 163, 124, 74, 73, 0)] == \
        [0, 0, 1, 1, 2, 2, 4, 4, 5, 5, 6, 7, 7]  # class 3 is empty: it shares class 2's threshold
    assert [M.block_parts(T, b) for b in (255, 218, 217, 210, 209, 0)] == [4, 4, 2, 2, 1, 1]
    none = M.Thresholds(T.thr, split_thr=256, split4_thr=256)
    assert [M.block_parts(none, b) for b in (255, 0)] == [1, 1]


def _class_sizes(T, buckets):
    return np.bincount([M.block_class(T, int(b)) for b in buckets], minlength=8).tolist()


def test_one_cell_per_bucket_160():
    """160 cells in buckets 24..183: the fractions 2, 5, 10, 20, 30, 50, 75 % of 160 are 3.2, 8, 16,
    32, 48, 80 and 120 cells, and a bucket with `above` cells above it is in the first class whose
    fraction exceeds `above`: sizes 4, 4, 8, 16, 16, 32, 40, 40."""
    _, b = distinct_costs(160)
    hist = np.bincount(b, minlength=256)
    T = M.next_thresholds(hist, 160, 160 // 25)
    assert T.thr == (180, 176, 168, 152, 136, 104, 64, 0)
    assert _class_sizes(T, b) == [4, 4, 8, 16, 16, 32, 40, 40]
    # 0.01f * 160f + 0.5f = 2.1: the two heaviest cells split in two
    assert (T.split_thr, T.split4_thr) == (182, 256)
    # the small-launch setting: 0.03f * 160f + 0.5f = 5.3 -> five cells four ways (15 of the 32
    # spare blocks); 0.10f * 160f + 0.5f = 16.5 -> the next eleven two ways (26 spare blocks in all)
    T = M.next_thresholds(hist, 160, 32, 0.10, 0.03)
    assert (T.split_thr, T.split4_thr) == (168, 179)
    # spare capacity cuts both ranges short: 3 * incl <= 7 -> two cells; then 6 + (incl - 2) <= 7
    T = M.next_thresholds(hist, 160, 7, 0.10, 0.03)
    assert (T.split_thr, T.split4_thr) == (181, 182)


def test_one_cell_per_bucket_200_float32():
    """200 cells in buckets 24..223. 0.30f * 200f rounds to 60.000004 in f32, so the bucket with
    exactly 60 cells above it stays in class 4: sizes 4, 6, 10, 20, 21, 39, 50, 50 (in exact
    arithmetic 20 and 40). The other products are exact."""
    _, b = distinct_costs(200)
    hist = np.bincount(b, minlength=256)
    T = M.next_thresholds(hist, 200, 8)
    assert T.thr == (220, 214, 204, 184, 163, 124, 74, 0)
    assert _class_sizes(T, b) == [4, 6, 10, 20, 21, 39, 50, 50]
    assert (T.split_thr, T.split4_thr) == (222, 256)  # 0.01f * 200f + 0.5f = 2.5
    T = M.next_thresholds(hist, 200, 40, 0.10, 0.03)
    assert (T.split_thr, T.split4_thr) == (204, 218)  # 6.5 -> six cells four ways; 20.5 -> twenty split


def test_float32_boundaries():
    f32 = np.float32
    assert f32(f32(0.01) * f32(50)) + f32(0.5) == f32(1.0)
    assert f32(0.02) * f32(100) == f32(2.0) and f32(0.02) * f32(200) == f32(4.0)
    # nb = 50, defaults: exactly the heaviest cell splits (incl = 1 <= 1.0)
    _, b = distinct_costs(50)
    T = M.next_thresholds(np.bincount(b, minlength=256), 50, 2)
    assert (T.split_thr, T.split4_thr) == (73, 256)
    # 2 % of 50 is one cell: the bucket with one cell above it is already class 1
    assert T.thr[:2] == (73, 71)
    # nb = 100: two cells in class 0 (above = 2 >= 2.0 ends it); nb = 200: four
    _, b = distinct_costs(100)
    assert M.next_thresholds(np.bincount(b, minlength=256), 100, 4).thr[0] == 122
    _, b = distinct_costs(200)
    assert M.next_thresholds(np.bincount(b, minlength=256), 200, 8).thr[0] == 220


def test_empty_classes_and_clamps():
    # all cells in one bucket: nothing above it -> class 0 from that bucket down, and too many to split
    hist = np.zeros(256, np.int64)
    hist[90] = 1000
    T = M.next_thresholds(hist, 1000, 40)
    assert T.thr == (90,) * 7 + (0,) and (T.split_thr, T.split4_thr) == (256, 256)
    # two levels, 10 % heavy: the heavy bucket is class 0; 100 cells lie above the light one, which
    # reaches the 2, 5 and 10 % fractions -> class 3; classes 1, 2 are empty and take thr[0], 4..6 thr[3]
    hist[:] = 0
    hist[140], hist[60] = 100, 900
    T = M.next_thresholds(hist, 1000, 200, 0.10, 0.03)
    assert T.thr == (140, 140, 140, 60, 60, 60, 60, 0)
    assert (T.split_thr, T.split4_thr) == (140, 256)  # 100 <= 100.5 and 100 <= 200; 100 > 30.5
    # all-zero costs: bucket 0 is class 0 (thr all 0); a split threshold of 0 is stored as 1
    hist[:] = 0
    hist[0] = 10
    assert M.next_thresholds(hist, 10, 40).thr == (0,) * 8
    T = M.next_thresholds(hist, 10, 40, 1.0, 1.0)
    assert (T.split_thr, T.split4_thr) == (1, 1)
    hist[0], hist[30] = 5, 5
    T = M.next_thresholds(hist, 10, 40, 1.0, 0.5)
    assert (T.split_thr, T.split4_thr) == (1, 30)


def test_plan_hand_worked():
    """Four blocks, thresholds by hand: block 2 (bucket 40) four ways, block 0 (bucket 32) two ways,
    both class 0; block 3 (bucket 24) class 1; block 1 (cost 0) class 7."""
    base = np.zeros(4, M.DBLOCK)
    base["x0"], base["y0"] = [0, 8, 16, 24], 8
    base["mask_lo"] = [0xFFFF00FF, FULL, 0x0001FFFF, 0x0F0F0F0F]
    base["mask_hi"] = [0x000000F0, FULL, 0x80000001, 0]
    base["out_base"] = [100, 128, 192, 212]
    base["flags"], base["base"], base["pad"] = [0, 1, 1, 0], [0, 1, 2, 3], [7, 0, 9, 0]
    T = M.Thresholds((32, 24, 24, 24, 24, 24, 24, 0), split_thr=32, split4_thr=40)
    out, used, nosplit = M.plan(base, np.array([16, 0, 32, 8], np.uint64), T, 5)
    assert (used, nosplit) == (8, 0)
    rows = [(b["x0"], b["mask_lo"], b["mask_hi"], b["out_base"], b["flags"], b["base"], b["pad"]) for b in out]
    assert rows == [(0, 0xFFFF00FF, 0, 100, 0, 0, 7), (0, 0, 0xF0, 124, 0, 0, 7),
                    (16, 0xFFFF, 0, 192, 1, 2, 9), (16, 0x00010000, 0, 208, 1, 2, 9),
                    (16, 0, 0x0001, 209, 1, 2, 9), (16, 0, 0x80000000, 210, 1, 2, 9),
                    (24, 0x0F0F0F0F, 0, 212, 0, 3, 0), (8, FULL, FULL, 128, 1, 1, 0), (0, 0, 0, 0, 0, 0, 0)]
    # one spare block too few: no splits at all, the class order stays
    out, used, nosplit = M.plan(base, np.array([16, 0, 32, 8], np.uint64), T, 3)
    assert (used, nosplit) == (4, 1) and out.size == 7
    assert out[:4].tobytes() == base[[0, 2, 3, 1]].tobytes() and not out[4:].tobytes().strip(b"\0")


@pytest.mark.parametrize("name", ["lognormal", "span", "ties", "two"])
@pytest.mark.parametrize("nb,max_split,split2,split4", [(1000, 40, -1.0, -1.0), (1000, 200, 0.10, 0.03),
                                                        (257, 1, -1.0, -1.0), (65, 13, 0.10, 0.03)])
def test_plan_properties(name, nb, max_split, split2, split4):
    """Random costs, thresholds from an earlier draw of the same distribution (the lag of one
    plan), every property checked block by block in plain Python."""
    rng = np.random.default_rng(nb * 131 + len(name))
    base = blocks(nb, rng)
    st = M.PlanState()
    for step in range(3):
        T = st.use
        cost = COSTS[name](rng, nb)
        out, used, nosplit = st.step(base, cost, max_split, split2, split4)
        assert out.size == nb + max_split and nb <= used <= nb + max_split
        assert not out[used:].tobytes().strip(b"\0")
        bkt = [M.cost_bucket(int(c)) for c in cost]
        seen = {}
        for i in range(used):
            seen.setdefault(int(out[i]["base"]), []).append(i)
        assert sorted(seen) == list(range(nb))  # a permutation of the base blocks, up to splitting
        for j, slots in seen.items():
            b = base[j]
            assert slots == list(range(slots[0], slots[0] + len(slots)))  # parts on consecutive slots
            whole = nosplit or T.split_thr == 0 or bkt[j] < T.split_thr
            want_parts = 1 if whole else (4 if bkt[j] >= T.split4_thr else 2)
            assert len(slots) == want_parts, (j, bkt[j], T)  # split exactly at or above the split bucket
            union, ob = 0, int(b["out_base"])
            for p, s in enumerate(slots):
                t = out[s]
                for f in ("x0", "y0", "flags", "base", "pad"):
                    assert t[f] == b[f]
                m = mask64(t)
                rows = 8 // len(slots)
                assert m == mask64(b) & (((1 << (8 * rows)) - 1) << (8 * rows * p))  # its row band
                assert union & m == 0 and int(t["out_base"]) == ob
                union |= m
                ob += bin(m).count("1")
            assert union == mask64(b)
        # graded: never a lighter bucket in an earlier class; base order inside a class
        cls = [M.block_class(T, bkt[int(out[i]["base"])]) for i in range(used)]
        assert cls == sorted(cls)
        for c in range(8):
            ids = [int(out[i]["base"]) for i in range(used) if cls[i] == c]
            assert ids == sorted(ids)
            later = [bkt[int(out[i]["base"])] for i in range(used) if cls[i] > c]
            if ids and later:
                assert min(bkt[j] for j in ids) >= max(later)
        if step and name == "lognormal" and max_split > 1:
            assert used > nb  # a smooth distribution's carried thresholds do split something


def test_state_lags_one_plan():
    """Plan n orders by the thresholds of plan n - 1's histogram: identity first, then the order of
    the first costs' thresholds applied to the second costs."""
    base = blocks(50)
    c0, b0 = distinct_costs(50)
    c1 = c0[::-1].copy()
    st = M.PlanState()
    out, used, nosplit = st.step(base, c0, 2)
    assert out[:50].tobytes() == base.tobytes() and (used, nosplit) == (50, 0)
    T = M.next_thresholds(np.bincount(b0, minlength=256), 50, 2)
    assert st.use == T
    out, used, nosplit = st.step(base, c1, 2)
    assert (used, nosplit) == (51, 0)  # the heaviest cell of c1, under c0's thresholds
    heavy = int(np.argmax(c1))
    assert out["base"][:2].tolist() == [heavy, heavy] and out["mask_hi"][:2].tolist() == [0, FULL]
    assert out.tobytes() == M.plan(base, c1, T, 2)[0].tobytes()
