"""atr_accumulate on the GPU: out.color, out.moments, out.length, variance and framebuffer for exact
equality with the plain C reference of tests/accumulate_ref.py (pinned without a GPU in
tests/test_accumulate_cpu.py), at the edges of the kernel's 64 x 4 blocks, for every subset of normal,
ident and moments, for a camera at rest, a small step, a quarter turn and a camera behind the surface,
through a chain of ping-ponged histories, in place, on two streams, and end to end on rendered frames with
render_guides and TemporalAccumulator; the arguments. Every raw output buffer is filled with a sentinel
first and guarded on both sides. Needs an MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import accumulate_ref as AR  # noqa: E402
from tests.test_accumulate_cpu import noisy, orbit, same, two_planes  # noqa: E402
from tests.test_gpu_parity import eng, run, upload  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F = np.float32
G = 256  # guard bytes around every raw output buffer
FILL = 0xAB
EMPTY = np.uint32(0xFFFFFFFF)
OUTS = (("color", 12, F, 3), ("moments", 8, F, 2), ("length", 4, np.uint32, 0), ("variance", 4, F, 0),
        ("framebuffer", 4, np.uint32, 0))
CENTER = (0, -15, -35)


def dev():
    return torch.device("cuda", 0)


def up(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev())


def raw(eng, color, guides, prev=None, moments=True, stream=None, mutate=None, **params):  # noqa: F811
    """atr_accumulate through ctypes on guarded, sentinel-filled buffers: (rc, the result as the
    reference's dict, or None). prev: the reference's dict with an atr_camera as "cam". mutate(args)
    may change the argument dict before the call."""
    h, w = color.shape[:2]
    n = h * w
    keep = [up(color)] + [up(a) for a in guides]
    buf = {k: torch.full((n * per + 2 * G,), FILL, dtype=torch.uint8, device=dev()) for k, per, _, _ in OUTS}
    addr = lambda a: a.data_ptr() if a is not None else None  # noqa: E731
    at = lambda k: buf[k].data_ptr() + G  # noqa: E731
    kw = dict(AR.DEFAULTS, **params)
    a = {"color": addr(keep[0]), "guides": E.atr_denoise_guides(*[addr(t) for t in keep[1:]]), "cam": None,
         "prev_guides": None, "prev": None, "w": w, "h": h,
         "params": E.atr_accumulate_params(kw["alpha"], kw["alpha_moments"], kw["max_length"], kw["plane_tolerance"],
                                           kw["min_normal_dot"]),
         "out": E.atr_history(at("color"), at("moments") if moments else None, at("length")),
         "variance": at("variance") if moments else None, "framebuffer": at("framebuffer")}
    if prev is not None:
        keep += [up(t) for t in prev["guides"]] + [up(prev["color"]), up(prev.get("moments")), up(prev["length"])]
        a["cam"] = prev["cam"]
        a["prev_guides"] = E.atr_denoise_guides(*[addr(t) for t in keep[4:7]])
        a["prev"] = E.atr_history(*[addr(t) for t in keep[7:10]])
    if mutate:
        mutate(a)
    ref = lambda s: C.byref(s) if s is not None else None  # noqa: E731
    torch.cuda.synchronize()
    rc = E.lib().atr_accumulate(eng.h, a["color"], ref(a["guides"]), ref(a["cam"]), ref(a["prev_guides"]), ref(a["prev"]),
                                a["w"], a["h"], ref(a["params"]), ref(a["out"]), a["variance"], a["framebuffer"],
                                C.c_void_p(stream) if stream else None)
    wrc, done = eng.wait()
    assert wrc == 0 and done == 0
    torch.cuda.synchronize()
    res = {}
    for k, per, dt, ch in OUTS:
        b = buf[k].cpu().numpy()
        assert (b[:G] == FILL).all() and (b[G + n * per:] == FILL).all(), (k, "guard bytes")
        body = b[G:G + n * per]
        written = rc == 0 and (moments or k not in ("moments", "variance"))
        if not written:
            assert (body == FILL).all(), (k, "written")
            res[k] = None
        else:
            res[k] = body.view(dt).reshape((h, w, ch) if ch else (h, w)).copy()
    return rc, (res if rc == 0 else None)


def check(eng, color, guides, prev=None, moments=True, **params):  # noqa: F811
    rc, out = raw(eng, color, guides, prev, moments, **params)
    assert rc == 0
    want = AR.accumulate(color, guides, prev, moments=moments, **params)
    for k, _, _, _ in OUTS:
        assert (out[k] is None) == (want[k] is None), k
        assert out[k] is None or AR.same_bits(out[k], want[k]), k
    return out


def pick(g, subset):
    return (g[0] if subset & 1 else None, g[1], g[2] if subset & 2 else None)


def cams(w, h, ks, step=0.01):
    return [E.camera(w, h, eye=e, facing=f) for e, f in (orbit(k, step, CENTER) for k in ks)]


def pair(eng, w, h, ks=(0, 1), step=0.01, subset=7, nan=True, seed=0, c=None, **params):  # noqa: F811
    """Two frames of the two-plane world from two cameras: starts a history, then accumulates into it."""
    c = c or cams(w, h, ks, step)
    g = [pick(two_planes(cam, nan=nan, seed=seed + i), subset) for i, cam in enumerate(c)]
    first = check(eng, noisy(h, w, seed + 10, nan=nan), g[0], None, moments=bool(subset & 4), **params)
    return check(eng, noisy(h, w, seed + 11, nan=nan), g[1], AR.history(first, c[0], g[0]), moments=bool(subset & 4),
                 **params), g[1]


# 63/64/65 and 3/4/5: one below, at and one above the kernel's block of 64 x 4 pixels
@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (5, 5), (63, 3), (64, 4), (65, 5), (64, 3), (65, 4), (129, 9),
                                 (130, 67)])
def test_sizes(eng, w, h):  # noqa: F811
    out, g = pair(eng, w, h, seed=w * 131 + h, alpha=0.1, alpha_moments=0.2)
    live = g[2] != EMPTY
    if live.sum() > 20:
        assert (out["length"] == 2).any()
    pair(eng, w, h, subset=0, nan=False, seed=w + h)


@pytest.mark.parametrize("subset", range(8))
def test_every_subset_of_normal_ident_and_moments(eng, subset):  # noqa: F811
    out, _ = pair(eng, 65, 33, subset=subset, seed=11)
    assert (out["length"] == 2).sum() > 100
    assert (out["moments"] is not None) == bool(subset & 4)


@pytest.mark.parametrize("name", ["at rest", "a small step", "a quarter turn", "behind"])
def test_camera_moves(eng, name):  # noqa: F811
    w, h = 97, 41
    if name != "behind":
        # the quarter turn is on the spot (78 degrees between the two facings), with a film of 35 degrees
        # to either side: only a strip at the film's edge reprojects, 13 % of the live pixels
        c = {"at rest": cams(w, h, (0, 0)), "a small step": cams(w, h, (0, 1), 0.02),
             "a quarter turn": [E.camera(w, h, h_fov=0.3), E.camera(w, h, h_fov=0.3, facing=(-1.0, -0.5, 0.1))]}[name]
        out, g = pair(eng, w, h, c=c, nan=False, seed=12)
        live = g[2] != EMPTY
        assert live.sum() > 500
        two = (out["length"] == 2).sum()
        if name == "at rest":
            assert (out["length"][live] == 2).all()
        elif name == "a small step":
            assert two > 0.8 * live.sum()
        else:
            assert 0 < two < 0.25 * live.sum() and (out["length"][live] == 1).any()
        return
    # the previous camera stands beyond the wall and looks the same way: every surface point is behind it
    cam = E.camera(w, h)
    far = E.camera(w, h, eye=(0.1, -20.0, -80.0))
    g = two_planes(cam, nan=False)
    first = check(eng, noisy(h, w, 1, nan=False), g, None)
    out = check(eng, noisy(h, w, 2, nan=False), g, AR.history(first, far, g))
    assert (out["length"][g[2] != EMPTY] == 1).all()


def test_a_chain_of_four_frames_through_two_histories(eng):  # noqa: F811
    """The engine's own ping-pong: frame f writes set f & 1 and reads the other."""
    w, h = 131, 37
    cs = cams(w, h, range(4), 0.01)
    sets = [{"color": torch.empty((h, w, 3), dtype=torch.float32, device=dev()),
             "moments": torch.empty((h, w, 2), dtype=torch.float32, device=dev()),
             "length": torch.empty((h, w), dtype=torch.int32, device=dev())} for _ in range(2)]
    prev = want = None
    for f, cam in enumerate(cs):
        g = two_planes(cam, seed=f)
        c = noisy(h, w, 50 + f)
        want = AR.accumulate(c, g, None if want is None else AR.history(want, cs[f - 1], gp), max_length=3)
        prev, var, fb = eng.accumulate(up(c), tuple(up(a) for a in g), prev, cam=cam, out=sets[f & 1], variance=True,
                                       framebuffer=True, max_length=3)
        rc, _ = eng.wait()
        assert rc == 0
        torch.cuda.synchronize()
        assert prev["color"].data_ptr() == sets[f & 1]["color"].data_ptr()
        got = {"color": prev["color"].cpu().numpy(), "moments": prev["moments"].cpu().numpy(),
               "length": prev["length"].cpu().numpy().view(np.uint32), "variance": var.cpu().numpy(),
               "framebuffer": fb.cpu().numpy().view(np.uint32)}
        assert same(got, want), f
        gp = g
    assert int(want["length"].max()) == 3 and (want["length"] == 3).sum() > 500


def test_in_place(eng):  # noqa: F811
    w, h = 101, 37
    c = cams(w, h, (0, 1))
    g = [two_planes(cam, seed=i) for i, cam in enumerate(c)]
    col = [noisy(h, w, 60), noisy(h, w, 61)]
    w0 = AR.accumulate(col[0], g[0], None, moments=False)
    w1 = AR.accumulate(col[1], g[1], AR.history(w0, c[0], g[0]), moments=False)
    t0, t1 = up(col[0]), up(col[1])
    h0 = eng.accumulate(t0, tuple(up(a) for a in g[0]), None, cam=c[0], moments=False, out={"color": t0})
    h1 = eng.accumulate(t1, tuple(up(a) for a in g[1]), h0, cam=c[1], out={"color": t1})  # out->color == color
    rc, _ = eng.wait()
    assert rc == 0
    torch.cuda.synchronize()
    assert h1["color"].data_ptr() == t1.data_ptr() and h1["moments"] is None
    assert AR.same_bits(t0.cpu().numpy(), w0["color"]) and AR.same_bits(t1.cpu().numpy(), w1["color"])
    assert np.array_equal(h1["length"].cpu().numpy().view(np.uint32), w1["length"])
    assert not AR.same_bits(w1["color"], col[1])


def test_two_streams(eng):  # noqa: F811
    sizes = [(50, 21), (333, 90)]
    data = []
    for i, (w, h) in enumerate(sizes):
        c = cams(w, h, (0, 1))
        g = [two_planes(cam, seed=i) for cam in c]
        col = [noisy(h, w, 70 + i), noisy(h, w, 80 + i)]
        data.append((c, g, col))
    s = [torch.cuda.Stream(device=dev()) for _ in sizes]
    tens = [([up(x) for x in col], [tuple(up(a) for a in gg) for gg in g]) for c, g, col in data]
    torch.cuda.synchronize()
    firsts = [eng.accumulate(tens[i][0][0], tens[i][1][0], None, cam=data[i][0][0], stream=s[i].cuda_stream)
              for i in range(2)]
    seconds = [eng.accumulate(tens[i][0][1], tens[i][1][1], firsts[i], cam=data[i][0][1], variance=True,
                              stream=s[i].cuda_stream) for i in range(2)]
    rc, done = eng.wait()
    assert rc == 0 and done == 0
    assert 0 < eng.last_kernel_ms() < 1000
    torch.cuda.synchronize()
    for i, (c, g, col) in enumerate(data):
        w0 = AR.accumulate(col[0], g[0], None)
        w1 = AR.accumulate(col[1], g[1], AR.history(w0, c[0], g[0]))
        hist, var = seconds[i]
        assert AR.same_bits(hist["color"].cpu().numpy(), w1["color"])
        assert AR.same_bits(hist["moments"].cpu().numpy(), w1["moments"])
        assert np.array_equal(hist["length"].cpu().numpy().view(np.uint32), w1["length"])
        assert AR.same_bits(var.cpu().numpy(), w1["variance"])


def test_invalid_arguments_leave_the_outputs_untouched(eng):  # noqa: F811
    w, h = 12, 9
    c = cams(w, h, (0, 1))
    g = [two_planes(cam, seed=i) for i, cam in enumerate(c)]
    first = AR.accumulate(noisy(h, w, 1), g[0], None)
    prev = AR.history(first, c[0], g[0])
    col = noisy(h, w, 2)
    inv = -1  # ATR_E_INVALID

    def bad(mutate=None, start=False, **kw):
        rc, _ = raw(eng, col, g[1], None if start else prev, mutate=mutate, **kw)  # raw() asserts the sentinels
        return rc

    def put(key, value=None):
        return lambda a: a.__setitem__(key, value)

    def field(key, name, value=None):
        return lambda a: setattr(a[key], name, value)

    assert bad() == 0 and bad(start=True) == 0
    for key in ("color", "params", "out", "cam", "prev_guides", "guides"):
        assert bad(put(key)) == inv, key
    for key in ("color", "params", "out"):
        assert bad(put(key), start=True) == inv, key
    assert bad(put("guides"), start=True) == 0  # no guides are needed to start a history
    for name in ("color", "length"):
        assert bad(field("out", name)) == inv and bad(field("prev", name)) == inv
    for size in [(0, 9), (12, 0), (-1, 9), (16385, 9), (12, 16385)]:
        assert bad(lambda a: a.update(w=size[0], h=size[1]), start=True) == inv
    assert bad(put("cam", E.camera(13, 9))) == inv and bad(put("cam", E.camera(12, 8))) == inv
    for k in (0.0, -1.0, float("nan"), float("inf")):
        cam = E.camera(w, h)
        cam.h_fov = k
        assert bad(put("cam", cam)) == inv
    for kw in [dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")), dict(alpha_moments=-0.1),
               dict(alpha_moments=1.5), dict(alpha_moments=float("nan")), dict(max_length=0),
               dict(max_length=(1 << 24) + 1), dict(plane_tolerance=0.0), dict(plane_tolerance=float("inf")),
               dict(plane_tolerance=float("nan")), dict(min_normal_dot=-1.5), dict(min_normal_dot=1.5),
               dict(min_normal_dot=float("nan"))]:
        assert bad(**kw) == inv, kw
        assert bad(start=True, **kw) == inv, kw
    assert bad(max_length=1 << 24) == 0 and bad(alpha=1.0, alpha_moments=1.0, min_normal_dot=-1.0) == 0
    for k in range(3):
        def res(a, k=k):
            a["params"].reserved[k] = 1
        assert bad(res) == inv
    # the pointer rules
    assert bad(field("guides", "position")) == inv and bad(field("prev_guides", "position")) == inv
    for name in ("normal", "ident"):
        assert bad(field("guides", name)) == inv and bad(field("prev_guides", name)) == inv
    assert bad(field("prev", "moments")) == inv
    assert bad(lambda a: (setattr(a["out"], "moments", None), a.update(variance=None))) == inv  # prev has moments
    assert bad(field("out", "moments"), start=True) == inv  # variance needs out->moments
    for name in ("color", "moments", "length"):
        assert bad(lambda a, name=name: setattr(a["out"], name, getattr(a["prev"], name))) == inv, name
    # NULL ctx
    p = E.atr_accumulate_params(0.0, 0.0, 64, 0.02, 0.9)
    o = torch.full((h * w * 3,), 7.0, dtype=torch.float32, device=dev())
    ln = torch.full((h * w,), 7, dtype=torch.int32, device=dev())
    ho = E.atr_history(o.data_ptr(), None, ln.data_ptr())
    t = up(col)
    assert E.lib().atr_accumulate(None, t.data_ptr(), None, None, None, None, w, h, C.byref(p), C.byref(ho), None, None,
                                  None) == inv
    torch.cuda.synchronize()
    assert (o == 7.0).all() and (ln == 7).all()
    with pytest.raises(ValueError):
        eng.accumulate(t.reshape(h, w * 3), None)
    with pytest.raises(ValueError):
        eng.accumulate(t, (t[:, :6].contiguous(), None, None))
    with pytest.raises(ValueError):
        eng.accumulate(t, (None, None, torch.zeros((h, w), dtype=torch.int64, device=dev())))
    with pytest.raises(ValueError):
        eng.accumulate(t.cpu(), None)
    with pytest.raises(ValueError):
        eng.accumulate(t, None, moments=False, variance=True)
    with pytest.raises(ValueError):
        eng.accumulate(t, None, prev={"cam": c[0]})
    with pytest.raises(ValueError):
        E.TemporalAccumulator(eng, radius=3)


def test_rendered_frames_with_their_guides_end_to_end(eng):  # noqa: F811
    """The Monkey at 72 x 40 from two consecutive cameras of the 0.02-rad orbit about its centre, 1 spp
    and 3 bounces, render_guides, TemporalAccumulator.push: the result equals the reference fed the same
    tensors, and at least 85 % of the second frame's live pixels found their history."""
    upload(eng, "Monkey")
    w, h = 72, 40
    acc = E.TemporalAccumulator(eng)
    want = prev = None
    for f in range(2):
        eye, facing = orbit(f, 0.02)
        cam = E.camera(w, h, 1, 3, eye=eye, facing=facing)
        frame = run(eng, cam)
        g = eng.render_guides(cam)
        color = torch.from_numpy(frame["rgb"]).to(dev())
        got, var = acc.push(cam, color, g if f else None)  # the first push renders the guides itself
        rc, _ = eng.wait()
        assert rc == 0
        torch.cuda.synchronize()
        gn = (g[0].cpu().numpy(), g[1].cpu().numpy(), g[2].cpu().numpy().view(np.uint32))
        want = AR.accumulate(frame["rgb"], gn, prev)
        prev = AR.history(want, cam, gn)
        assert AR.same_bits(got.cpu().numpy(), want["color"]), f
        assert AR.same_bits(var.cpu().numpy(), want["variance"]), f
        assert np.array_equal(acc.prev["length"].cpu().numpy().view(np.uint32), want["length"]), f
        assert AR.same_bits(acc.prev["moments"].cpu().numpy(), want["moments"]), f
    hit = frame["face"] != E.MISS
    assert 100 < hit.sum() < hit.size and np.array_equal(want["length"] == 0, ~hit)
    found = (want["length"][hit] == 2).mean()
    print(f"{int(hit.sum())} live pixels, {100 * found:.1f} % with length 2")
    assert found >= 0.85
    assert not AR.same_bits(want["color"][hit], frame["rgb"][hit])
    acc.reset()
    got, _ = acc.push(cam, color, g)
    rc, _ = eng.wait()
    assert rc == 0
    torch.cuda.synchronize()
    assert AR.same_bits(got.cpu().numpy(), frame["rgb"])
