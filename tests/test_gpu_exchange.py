"""The frame-exchange kernels (exchange.hip: atr_pack_bgr*, atr_scatter_bgr*, atr_unpack_masked*)
on synthetic frames at their edges, bit for bit against the host references of atray_amd/shard.py
and the slot -> pixel map of atr_packed_pixel_map. No scene, no render, no oracle: the operations
are byte shuffles. Needs an MI355X (-m gpu).

Buffers are laid out so that a wrong kernel fails a comparison instead of leaving its memory: a
source is allocated to whole 8192-pixel chunks and holds non-background pixels from n on (a count
that ignores i < n changes the stream), a stream buffer is the bound of the whole chunks plus 64
bytes of 0xA5 that must survive, an index's tail points at the image's slack, and images carry the
sentinel 0x7F7F7F7F wherever no source owns a pixel."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd import shard as S  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = S.MASK_CHUNK
SENT = 0x7F7F7F7F
FILL = 0xA5
COMMON = 0x00EBCE87  # "a common colour": any value a pixel can have
ABSENT = 0x01000000  # a non-zero X byte: no pixel can equal it
BACKGROUNDS = (0, COMMON, ABSENT)
PATTERNS = ("allbg", "nobg", "d14", "d50", "first", "last", "groups", "words")


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = E.Engine(0)
    yield e
    e.close()


def _chunks(n):
    return -(-n // CHUNK)


def _keep(rng, n, pattern):
    """True where the pixel is not the background."""
    i = np.arange(n)
    if pattern == "allbg":
        return np.zeros(n, bool)
    if pattern == "nobg":
        return np.ones(n, bool)
    if pattern in ("d14", "d50"):  # 0.14: a c3 frame (86% sky)
        return rng.random(n) < (0.14 if pattern == "d14" else 0.5)
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == n - 1
    if pattern == "groups":  # full 64-pixel groups next to empty ones
        return ((i >> 6) & 1) == 0
    if pattern == "words":  # full 32-bit mask words next to empty ones
        return ((i >> 5) & 1) == 0
    if pattern == "lastchunk":  # only the last chunk holds payload: every earlier offset is 0
        return i >= (_chunks(n) - 1) * CHUNK
    raise KeyError(pattern)


def _source(rng, n, keep, bg):
    """BGRX pixels (X byte 0) to whole chunks: the background stamped over [0, n) where keep is
    false, non-background values everywhere else (from n on too). For the background no pixel can
    equal (X byte set) the stamp is 0, its low 24 bits: every pixel then travels, and an encoder
    that compared 24 bits only would drop these."""
    full = rng.integers(0, 1 << 24, max(_chunks(n), 1) * CHUNK, dtype=np.uint32)
    full[full == bg] ^= 1
    full[:n][~keep] = bg if bg < (1 << 24) else 0
    return full


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return (torch.from_numpy(a) if a.flags.writeable else torch.tensor(a)).cuda()  # shared cases are read-only


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _encode(eng, full, n, bg):
    """atr_pack_bgr_masked of full[:n] -> (the whole out buffer, the device's nbytes)."""
    src = _dev(full)
    out = torch.full((E.pack_bgr_masked_bound(_chunks(n) * CHUNK) + 64,), FILL, dtype=torch.uint8, device="cuda")
    nbytes = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    eng.pack_bgr_masked(src.data_ptr(), n, bg, out.data_ptr(), nbytes.data_ptr())
    torch.cuda.synchronize()
    return out, int(nbytes.item())


def _check_stream(out, nbytes, want, what):
    assert nbytes == want.size, (what, nbytes, want.size)
    got = out.cpu().numpy()
    bad = np.flatnonzero(got[:want.size] != want)
    assert bad.size == 0, (what, "first wrong byte", int(bad[0]), "of", want.size, "wrong bytes", int(bad.size))
    assert (got[want.size:] == FILL).all(), (what, "bytes written past nbytes")


def _padded_stream(want):
    """A host-made stream uploaded, with 64 bytes of slack after it."""
    return _dev(np.concatenate([want, np.full(64, FILL, np.uint8)]))


@functools.lru_cache(maxsize=4)
def _scatter_index(n):
    """A random injection of [0, n) into an image of n + slack pixels (slack 5..64), as an index to
    whole chunks whose tail points at the slack: (index, image size). Shared, read-only."""
    size = n + 5 + n % 60
    perm = np.random.default_rng(1000003 + n).permutation(size).astype(np.int64)
    idx = np.empty(max(_chunks(n), 1) * CHUNK, np.int64)
    idx[:n] = perm[:n]
    idx[n:] = np.resize(perm[n:], idx.size - n)
    idx.setflags(write=False)
    return idx, size


def _check_masked_scatter(eng, stream, n, pixels, what):
    """atr_scatter_bgr_masked of a device stream through _scatter_index: the image holds `pixels`
    where the index points and the sentinel elsewhere."""
    idx, size = _scatter_index(n)
    didx = _dev(idx)
    img = torch.full((size,), SENT, dtype=torch.int32, device="cuda")
    eng.scatter_bgr_masked(stream.data_ptr(), n, didx.data_ptr(), img.data_ptr())
    torch.cuda.synchronize()
    got = _u32(img)
    owned = np.zeros(size, bool)
    owned[idx[:n]] = True
    bad = np.flatnonzero(got[idx[:n]] != pixels)
    assert bad.size == 0, (what, "first wrong pixel", int(bad[0]), "wrong pixels", int(bad.size), "of", n)
    assert (got[~owned] == SENT).all(), (what, "a pixel no source owns was written")


# ------------------------------------------------------------------ (a) atr_pack_bgr / atr_scatter_bgr
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 100003])
def test_pack_and_scatter_bgr_match_host(eng, n):
    """atr_pack_bgr at sizes around the 64-lane wave and the 256-thread block: the bytes equal
    pack_bgr_host and nothing is written past 3 n; atr_scatter_bgr of those bytes through a random
    injection into a larger image equals scatter_bgr_host, every other pixel still the sentinel."""
    rng = np.random.default_rng(n)
    pad = -(-n // 256) * 256  # to whole blocks, so an unguarded tail lane stays inside the buffers
    px = rng.integers(0, 1 << 24, pad, dtype=np.uint32)
    src = _dev(px)
    out = torch.full((3 * pad + 64,), FILL, dtype=torch.uint8, device="cuda")
    eng.pack_bgr(src.data_ptr(), n, out.data_ptr())
    torch.cuda.synchronize()
    want = S.pack_bgr_host(px[:n])
    got = out.cpu().numpy()
    assert np.array_equal(got[:3 * n], want)
    assert (got[3 * n:] == FILL).all()

    size = n + 5 + n % 60
    perm = rng.permutation(size).astype(np.int64)
    idx = np.empty(pad, np.int64)
    idx[:n] = perm[:n]
    idx[n:] = np.resize(perm[n:], pad - n)  # an unguarded tail lane would write the slack
    didx = _dev(idx)
    img = torch.full((size,), SENT, dtype=torch.int32, device="cuda")
    packed = _dev(np.concatenate([want, np.full(3 * (pad - n) + 64, FILL, np.uint8)]))
    eng.scatter_bgr(packed.data_ptr(), n, didx.data_ptr(), img.data_ptr())
    torch.cuda.synchronize()
    exp = np.full(size, SENT, np.uint32)
    S.scatter_bgr_host(want, idx[:n], exp)
    assert np.array_equal(exp[idx[:n]], px[:n])  # the host reference inverts the host packing
    assert np.array_equal(_u32(img), exp)


# ------------------------------------------------------------------ (b), (d) the masked stream
MASKED_SIZES = [0, 1, 63, 64, 65, 2047, 2048, 2049, 8191, 8192, 8193, 3 * 8192 + 1]


def _masked_case(n, pattern, bg):
    rng = np.random.default_rng([n, PATTERNS.index(pattern), BACKGROUNDS.index(bg)])
    return _source(rng, n, _keep(rng, n, pattern), bg)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", MASKED_SIZES)
def test_pack_bgr_masked_matches_host(eng, n, pattern):
    """atr_pack_bgr_masked at the tails of a 64-pixel group, a 2048-pixel wave span and an
    8192-pixel chunk (n = 0: the header only), under every mask pattern and background: the
    device's byte count is the host stream's length, the bytes are pack_bgr_masked_host's, and
    nothing is written past them."""
    for bg in BACKGROUNDS:
        full = _masked_case(n, pattern, bg)
        want = S.pack_bgr_masked_host(full[:n], bg)
        out, nbytes = _encode(eng, full, n, bg)
        _check_stream(out, nbytes, want, f"bg={bg:#x}")


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", MASKED_SIZES)
def test_scatter_bgr_masked_decodes_device_and_host_streams(eng, n, pattern):
    """atr_scatter_bgr_masked of the streams above, the device-made one and the host reference's
    uploaded (so that an encoder's and a decoder's error cannot cancel), through a random injection
    into a sentinel image: the source frame comes back and no other pixel is written."""
    for bg in BACKGROUNDS:
        full = _masked_case(n, pattern, bg)
        out, _ = _encode(eng, full, n, bg)
        _check_masked_scatter(eng, out, n, full[:n], f"device stream, bg={bg:#x}")
        host = _padded_stream(S.pack_bgr_masked_host(full[:n], bg))
        _check_masked_scatter(eng, host, n, full[:n], f"host stream, bg={bg:#x}")


# ------------------------------------------------------------------ (c) the scan's carry
# masked_scan_kernel scans 1024 chunk counts per pass: 1024 chunks is the last single pass, one
# pixel more the first carry, 1026 chunks less 37 pixels a carry into a pass with a ragged end.
SCAN_CASES = [(1024 * 8192, "d14"), (1024 * 8192 + 1, "d14"), (1026 * 8192 - 37, "d14"),
              (1024 * 8192 + 1, "lastchunk"), (1026 * 8192 - 37, "lastchunk")]


@functools.lru_cache(maxsize=None)
def _scan_case(n, pattern):
    """(source to whole chunks, host stream) of a scan case: computed once, shared, read-only."""
    rng = np.random.default_rng([n, len(pattern)])
    keep = _keep(rng, n, pattern)
    keep[n - 1] = True  # the last chunk always holds payload, whose place depends on the carry
    full = _source(rng, n, keep, COMMON)
    want = S.pack_bgr_masked_host(full[:n], COMMON)
    full.setflags(write=False)
    want.setflags(write=False)
    return full, want


@pytest.mark.parametrize("n,pattern", SCAN_CASES)
def test_masked_scan_carries_past_1024_chunks(eng, n, pattern):
    """More than 1024 chunks (8,388,608 pixels): the chunk offsets of the scan's second pass and the
    header's total carry the first pass's sum. 'lastchunk' has payload in the last chunk only, so
    every earlier offset is 0 and the total is the carry alone."""
    full, want = _scan_case(n, pattern)
    out, nbytes = _encode(eng, full, n, COMMON)
    _check_stream(out, nbytes, want, f"n={n}")


@pytest.mark.parametrize("n,pattern", SCAN_CASES)
def test_scatter_bgr_masked_past_1024_chunks(eng, n, pattern):
    """The scan cases' streams, device-made and host-made, decoded by atr_scatter_bgr_masked."""
    full, want = _scan_case(n, pattern)
    out, _ = _encode(eng, full, n, COMMON)
    _check_masked_scatter(eng, out, n, full[:n], "device stream")
    del out
    _check_masked_scatter(eng, _padded_stream(want), n, full[:n], "host stream")


# ------------------------------------------------------------------ (e) atr_unpack_masked
UW, UH = 77, 45  # neither a multiple of 8: partial blocks on the right and top edges
UNPACK_LISTS = ("full", "rect", "three", "column", "shard0", "shard1", "shard2")
UNPACK_FRAMES = (1, 3, 4, 5, 9)  # the kernel takes 4 frames at a time


def _unpack_tiles(name):
    if name.startswith("shard"):
        return np.asarray(S.ShardPlan(UW, UH, 3, 32).tiles[int(name[5:])]).reshape(-1, 4).tolist()
    return {"full": [[0, 0, UW - 1, UH - 1]],
            "rect": [[3, 5, 40, 33]],
            "three": [[3, 5, 40, 33], [70, 0, 76, 44], [50, 40, 50, 40]],
            "column": [[61, 2, 61, 43]]}[name]


def _frames_source(rng, npix, bg=COMMON, density=0.5):
    return _source(rng, npix, rng.random(npix) < density, bg)


def _expected_frames(src, pmap, nframes, stride, size):
    own = pmap.size
    exp = np.full(size, SENT, np.uint32)
    for f in range(nframes):
        exp[f * stride + pmap] = src[f * own:(f + 1) * own]
    return exp


def _check_unpack_masked(eng, name, nframes):
    tiles = _unpack_tiles(name)
    pmap = E.packed_pixel_map(tiles, UW, UH)
    own = pmap.size
    assert own == E.packed_size(tiles) and np.unique(pmap).size == own
    rng = np.random.default_rng([UNPACK_LISTS.index(name), nframes])
    full = _frames_source(rng, nframes * own)  # nframes x own pixels, contiguous
    want = S.pack_bgr_masked_host(full[:nframes * own], COMMON)
    dev_stream, nbytes = _encode(eng, full, nframes * own, COMMON)
    assert nbytes == want.size
    host_stream = _padded_stream(want)
    for stride in (UW * UH, UW * UH + 5):
        size = nframes * stride + 7
        exp = _expected_frames(full, pmap, nframes, stride, size)
        for what, stream in (("host stream", host_stream), ("device stream", dev_stream)):
            img = torch.full((size,), SENT, dtype=torch.int32, device="cuda")
            eng.unpack_masked(tiles, UW, UH, stream.data_ptr(), nframes, img.data_ptr(), stride)
            torch.cuda.synchronize()
            got = _u32(img)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (what, "stride", stride, "first wrong element", int(bad[0]), "wrong", int(bad.size),
                                   "written outside the tiles", int((exp[bad] == SENT).sum()))


def test_unpack_masked_cases_cover_the_unaligned_paths():
    """The lists below hold what the kernel's unaligned paths need: a per-frame pixel count that is
    no multiple of 64 (a block's slots straddle two mask groups, and from frame 1 on nothing is
    aligned) and frames that cross an 8192-pixel chunk."""
    own = {name: E.packed_size(_unpack_tiles(name)) for name in UNPACK_LISTS}
    assert own["full"] == UW * UH and own["full"] % 64 != 0 and own["rect"] % 64 != 0
    assert 5 * own["full"] > 2 * CHUNK and 9 in UNPACK_FRAMES
    assert own["three"] == 38 * 29 + 7 * 45 + 1 and own["column"] == 42
    assert sum(own[f"shard{r}"] for r in range(3)) == UW * UH


@pytest.mark.parametrize("nframes", UNPACK_FRAMES)
@pytest.mark.parametrize("name", UNPACK_LISTS)
def test_unpack_masked_matches_pixel_map(eng, name, nframes):
    """atr_unpack_masked on a 77x45 image: rects unaligned to 8, one-pixel rects, edge blocks with
    partial masks, frame counts around the kernel's 4 at a time, frames W * H and W * H + 5 apart;
    image[f * stride + map[slot]] = src[f * own + slot] for the host reference's stream and the
    device encoder's, and every other element keeps the sentinel."""
    _check_unpack_masked(eng, name, nframes)


@pytest.mark.parametrize("nframes", UNPACK_FRAMES)
@pytest.mark.parametrize("name", UNPACK_LISTS)
def test_unpack_masked_under_cell_plan(eng, name, nframes):
    """The same with a cell plan set: blocks split into 2, 4 or 8 row bands, reordered by dispatch
    class and flagged for priority keep their packed slots (out_base), so the result is the
    plan-less one."""
    rng = np.random.default_rng([7, UNPACK_LISTS.index(name), nframes])
    cells = ((UW + 7) // 8) * ((UH + 7) // 8)
    plan = (rng.choice([0, 2, 4, 8], cells) | (rng.integers(0, 8, cells) << 4) |
            (rng.integers(0, 2, cells) * E.ATR_PLAN_PRIO)).astype(np.uint8)
    eng.set_cell_plan(UW, UH, plan)
    try:
        _check_unpack_masked(eng, name, nframes)
    finally:
        eng.set_cell_plan(UW, UH, None)


# ------------------------------------------------------------------ (f) atr_unpack_masked_ranks
RW, RH = 256, 64


def test_unpack_masked_ranks_mixed_sources(eng):
    """20 disjoint sources in one call (two decode launches: 16 + 4), 3 frames W * H + 5 apart:
    17 streams, two raw u32 frame sets (one per launch) and an empty rect. The image equals the
    per-source atr_unpack_masked result and the map-based expectation."""
    F, stride = 3, RW * RH + 5
    size = F * stride + 9
    rng = np.random.default_rng(20)
    edges = [round(RW * k / 19) for k in range(20)]  # 19 strips, 13 or 14 pixels wide
    lists = []
    for k in range(19):
        x0, x1 = edges[k], edges[k + 1] - 1
        lists.append([[x0, 0, x1, RH - 1]] if k % 2 == 0 else [[x0, 31, x1, RH - 1], [x0, 0, x1, 30]])
    lists.insert(7, [[0, 0, -1, -1]])  # a source without pixels
    raw = [int(i in (3, 18)) for i in range(20)]
    exp = np.full(size, SENT, np.uint32)
    each = torch.full((size,), SENT, dtype=torch.int32, device="cuda")
    keep, ptrs = [], []
    for i, tiles in enumerate(lists):
        if i == 7:
            ptrs.append(keep[0].data_ptr())  # any valid pointer: nothing is read
            continue
        pmap = E.packed_pixel_map(tiles, RW, RH)
        own = pmap.size
        full = _frames_source(rng, F * own)
        exp_i = _expected_frames(full, pmap, F, stride, size)
        assert (exp[exp_i != SENT] == SENT).all()  # disjoint
        exp[exp_i != SENT] = exp_i[exp_i != SENT]
        stream = _padded_stream(S.pack_bgr_masked_host(full[:F * own], COMMON))
        eng.unpack_masked(tiles, RW, RH, stream.data_ptr(), F, each.data_ptr(), stride)
        src = _dev(full) if raw[i] else stream
        keep += [stream, src]
        ptrs.append(src.data_ptr())
    assert (exp.reshape(-1)[:F * stride].reshape(F, stride)[:, :RW * RH] != SENT).all()  # the strips tile the image
    img = torch.full((size,), SENT, dtype=torch.int32, device="cuda")
    eng.unpack_masked_ranks(lists, RW, RH, ptrs, F, img.data_ptr(), stride, raw=raw)
    torch.cuda.synchronize()
    assert np.array_equal(_u32(each), exp)
    assert np.array_equal(_u32(img), exp)


def test_exchange_entry_points_reject_bad_arguments(eng):
    """image_stride below W * H and negative pixel counts return ATR_E_INVALID (nothing is
    launched)."""
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    idx = torch.zeros(16, dtype=torch.int64, device="cuda")
    p, tiles = buf.data_ptr(), [[0, 0, 7, 7]]
    with pytest.raises(E.AtrError, match="ATR_E_INVALID"):
        eng.unpack_masked(tiles, 8, 8, p, 1, p, 63)
    with pytest.raises(E.AtrError, match="ATR_E_INVALID"):
        eng.unpack_masked_ranks([tiles], 8, 8, [p], 1, p, 63)
    with pytest.raises(E.AtrError, match="ATR_E_INVALID"):
        eng.pack_bgr(p, -1, p)
    with pytest.raises(E.AtrError, match="ATR_E_INVALID"):
        eng.scatter_bgr(p, -1, idx.data_ptr(), p)
    with pytest.raises(E.AtrError, match="ATR_E_INVALID"):
        eng.pack_bgr_masked(p, -1, 0, p, idx.data_ptr())
    with pytest.raises(E.AtrError, match="ATR_E_INVALID"):
        eng.scatter_bgr_masked(p, -1, idx.data_ptr(), p)
    assert E.pack_bgr_masked_bound(-1) < 0
    torch.cuda.synchronize()
    assert not buf.any()


# ------------------------------------------------------------------ (g) the block cache's eviction race
# Device work the context knows nothing about, enqueued ahead of the call so that its decodes wait
# while its host side runs (32 small copies; the whole test takes 0.02 s without the sleep). The aim
# is 20 to 100 ms; once the launches are recorded the result no longer depends on it.
SLEEP_CYCLES = 120_000_000  # torch.cuda._sleep: 50.0 ms between two events on an MI355X (51.2, 50.0, 50.0)


def test_unpack_masked_ranks_eviction_waits_for_earlier_batch():
    """atr_unpack_masked_ranks with more sources (32) than the block cache holds (24), on a fresh
    context and a non-blocking stream that is still busy: the second batch's cache misses evict
    block sets of the first batch, whose decode has not run yet, so the context must have recorded
    that launch before it rewrites them. Every source is one 8-aligned 32x32 rect (the rects tile a
    256x128 image), so all block lists have the same length, masks and slots: a decode that read
    another list's blocks would stay inside every buffer and write its pixels to the wrong rect
    (once the race is lost, the rects of sources 0 to 7 keep the sentinel)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    W, H, side = 256, 128, 32
    rng = np.random.default_rng(32)
    lists = [[[x, y, x + side - 1, y + side - 1]] for y in range(0, H, side) for x in range(0, W, side)]
    assert len(lists) == 32
    exp = np.full(W * H + 11, SENT, np.uint32)
    streams, maps = [], []
    for tiles in lists:
        pmap = E.packed_pixel_map(tiles, W, H)
        full = _frames_source(rng, pmap.size)
        exp[pmap] = full[:pmap.size]
        maps.append(pmap)
        streams.append(_padded_stream(S.pack_bgr_masked_host(full[:pmap.size], COMMON)))
    img = torch.full((exp.size,), SENT, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    own = E.Engine(0)  # its 24 cache slots are empty
    try:
        st = torch.cuda.Stream()  # a non-blocking pool stream: host copies do not serialise with it
        with torch.cuda.stream(st):
            torch.cuda._sleep(SLEEP_CYCLES)
        own.unpack_masked_ranks(lists, W, H, [t.data_ptr() for t in streams], 1, img.data_ptr(), W * H,
                                stream=st.cuda_stream)
        torch.cuda.synchronize()
    finally:
        own.close()
    got = _u32(img)
    wrong = [i for i, m in enumerate(maps) if not np.array_equal(got[m], exp[m])]
    untouched = [i for i, m in enumerate(maps) if (got[m] == SENT).all()]
    assert not wrong, f"sources with wrong pixels: {wrong}, of which still at the sentinel: {untouched}"
    assert np.array_equal(got, exp)
