"""atr_radiance_rays, atr_gather_radiance and atr_probe_sh through the host flow they share, held to the
same bracket: the three calls one after the other on one context, in batches of 2^12 paths (three
batches of one group of rays, the last holding one ray; two batches of points, the last holding one),
once each alone with a wait between and once back to back with the middle call on a second stream --
the same bits both times, the references' bits (the helpers and references of the three calls' own test
files), a wait and a time after every lone call, an unchanged render around it all; and the order of the
three calls' argument checks. Needs an MI355X (-m gpu)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import gather_radiance_ref as GRR  # noqa: E402
from tests import probe_sh_ref as PR  # noqa: E402
from tests import radiance_ref as RR  # noqa: E402
from tests import test_gpu_gather_radiance as GG  # noqa: E402
from tests import test_gpu_probe_sh as GP  # noqa: E402
from tests import test_gpu_radiance as GRAD  # noqa: E402
from tests import test_probe_sh_cpu as PC  # noqa: E402
from tests import test_radiance_cpu as RC  # noqa: E402
from tests.test_gather_cpu import points  # noqa: E402
from tests.test_gpu_parity import eng, run  # noqa: E402,F401
from tests.test_gpu_scenes import MIXED  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SEED = RC.SEED
BL = 3
MODS = (GRAD, GG, GP)  # the calls in the sequence's order: raw_call(eng, *arrays, n, ns, bl, out, ...)
SHAPES = ((129, 64), (3, 2048), (3, 2048))  # items x samples: rays, points, probes


def dev():
    return torch.device("cuda", 0)


def inputs():
    """The arrays of the three calls: rays (origins, directions), points (positions, normals), probes."""
    (n0, _), (n1, _), (n2, _) = SHAPES
    return (tuple(a[:n0] for a in RC.batch("mixed", "second")), tuple(a[:n1] for a in points("mixed")),
            (PC.probes("mixed")[:n2],))


@functools.lru_cache(maxsize=None)
def refs():
    """The references of the three calls, computed once; the queue order changes no output."""
    (o, d), (p, n), (q,) = inputs()
    sc = MIXED.oracle()
    return (RR.radiance(sc, o, d, SHAPES[0][1], BL, SEED), GRR.gather_radiance(sc, p, n, SHAPES[1][1], BL, SEED),
            PR.probe_sh(sc, q, SHAPES[2][1], BL, SEED))


def bufs(i, n, ns):
    return MODS[i].Bufs(n) if i == 0 else MODS[i].Bufs(n, ns)


def sequence(eng, sb, lone):
    """The three calls into guarded buffers made beforehand. lone: each on torch's current stream with
    a wait and a time after it; else back to back with no wait, the middle one on a stream of its own."""
    arrays = [tuple(torch.from_numpy(np.array(a, F)).to(dev()) for a in arrs) for arrs in inputs()]
    out = [bufs(i, n, ns) for i, (n, ns) in enumerate(SHAPES)]
    second = torch.cuda.Stream(dev())
    torch.cuda.synchronize()  # the fills and copies above, ahead of a call on another stream
    for i, (n, ns) in enumerate(SHAPES):
        stream = second.cuda_stream if i == 1 and not lone else None
        assert MODS[i].raw_call(eng, *arrays[i], n, ns, BL, out[i].out(), sort_bits=sb, stream=stream) == 0, i
        if lone:
            assert eng.wait() == (0, 0), i
            assert eng.last_kernel_ms() > 0, i
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    return [MODS[i].host(b) for i, b in enumerate(out)]


@pytest.mark.parametrize("sb", [0, 2])
def test_the_three_calls_in_sequence(eng, sb):
    MIXED.upload(eng)
    base = eng.tuning()
    cam = E.camera(64, 64, 1, 1)
    try:
        eng.set_tuning(path_batch_log2=12)
        for (n, ns), unit in zip(SHAPES, (64, 1, 1)):  # batches of whole groups of 64 rays, points, probes
            assert (n + unit - 1) // unit > max(1, 4096 // (unit * ns))  # more than one batch
        before = run(eng, cam)
        alone = sequence(eng, sb, lone=True)
        together = sequence(eng, sb, lone=False)
        after = run(eng, cam)
    finally:
        eng.set_tuning(**base)
    for i, (a, b) in enumerate(zip(alone, together)):
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(a[k], b[k]), (i, k, sb)
    wr, wg, wp = refs()
    GRAD.same(together[0], wr, ("radiance", sb))
    GG.same(together[1], wg, ("gather", sb))
    GP.same(together[2], wp, ("probes", sb), traced=wp["traced"])
    for k in before:
        assert np.array_equal(before[k], after[k]), ("render", k, sb)


@pytest.mark.parametrize("i", [0, 1, 2], ids=["radiance", "gather", "probes"])
def test_the_order_of_the_argument_checks(eng, i):
    """Every ATR_E_INVALID cause before ATR_E_NOSCENE, that before the early ATR_OK of an empty call;
    a continued range without its sum is refused even when the call is empty."""
    MIXED.upload(eng)
    n, ns = 9, 3
    arrays = tuple(torch.from_numpy(np.array(a[:n], F)).to(dev()) for a in inputs()[i])
    none = (None,) * len(arrays)
    b = bufs(i, n, ns)
    raw = MODS[i].raw_call
    assert raw(eng, *none, 0, ns, BL, b.out()) == 0
    assert raw(eng, *none, 0, ns, BL, b.out([k for k in MODS[i].ALL if k != "sum"]), first=1) == -1
    torch.cuda.synchronize()
    for k in MODS[i].ALL:
        assert (b.get(k).view(np.uint8) == MODS[i].FILL).all(), k
    assert int(b.traced.item()) == 5  # nothing was written
    fresh = E.Engine(0)
    try:
        assert raw(fresh, *arrays, n, ns, BL, b.out()) == -4  # ATR_E_NOSCENE
        assert raw(fresh, *arrays, n, ns, BL, b.out(), sort_bits=1) == -1
    finally:
        fresh.close()
