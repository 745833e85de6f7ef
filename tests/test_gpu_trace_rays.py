"""atr_trace_rays on the GPU against the oracle's own ray queries (oracle.Scene.trace on composed
scenes): the bits of t, face and (u, v) for every kernel variant and batch order; model, kind and
material derived from oracle traces of the scene's parts; the normal against a numpy-f32
restatement of shade.h; invalid rays; order independence; partial outputs, streams, arguments and
workspace growth. Needs an MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests.goldens import SEED  # noqa: E402
from tests.test_gpu_parity import eng, run  # noqa: E402,F401
from tests.test_gpu_scenes import MATS, MIXED, PLANES, SOUP_SC, SPHERES, TIES, Sc, ref  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
VARIANTS = (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_LANE)
SORTS = (0, 2, 5, 7)
NOMODEL = Sc([], [], MATS, SPHERES + [((0.3, 0.6, -3.0), 0.7, 3)], PLANES)
SCENES = {"mixed": MIXED, "ties": TIES[0], "soup": SOUP_SC, "nomodel": NOMODEL}
NOMODEL_BOX = np.array([-2.5, -0.5, -4.5, 1.5, 2.5, -2.0], F)  # around its two spheres
N_BIG, N_SMALL = 4097, 1025

_boxes, _rays, _traces = {}, {}, {}


def sphere_box(s):
    (cx, cy, cz), r, _ = s
    return np.array([cx - r, cy - r, cz - r, cx + r, cy + r, cz + r], F)


def boxes(name):
    """[the scene box, each model's box, each sphere's box] of a scene (the scene box alone first)."""
    if name not in _boxes:
        sc = SCENES[name]
        parts = [np.asarray(p.surrounding_aabb, F) for p in sc.parts()]
        if parts:
            lo = np.min([b[:3] for b in parts], axis=0)
            hi = np.max([b[3:] for b in parts], axis=0)
            whole = np.concatenate([lo, hi]).astype(F)
        else:
            whole = NOMODEL_BOX
        _boxes[name] = [whole] + parts + [sphere_box(s) for s in sc.spheres]
    return _boxes[name]


def focus(name):
    """The box of the `inside` rays: the Monkey's where the scene has one, else the scene box."""
    sc = SCENES[name]
    return boxes(name)[1 + sc.names.index("monkey")] if "monkey" in sc.names else boxes(name)[0]


def trace(name, orig, dirs, key=None):
    """The oracle's trace of a batch on a scene (cached under key, read-only)."""
    if key is not None and (name, key) in _traces:
        return _traces[name, key]
    face, t, uv, _ = SCENES[name].oracle().trace(orig, dirs)
    for a in (face, t, uv):
        a.setflags(write=False)
    if key is not None:
        _traces[name, key] = (face, t, uv)
    return face, t, uv


def rays(name, kind):
    """A named batch of a scene (cached, read-only): (orig, dirs)."""
    if (name, kind) not in _rays:
        if kind == "aimed":
            o, d = R.aimed(boxes(name), N_BIG, 21)
        elif kind == "second":
            ao, ad = rays(name, "aimed")
            o, d = R.second_generation(ao, ad, trace(name, ao, ad, "aimed")[1], 22, N_SMALL)
        elif kind == "axis":
            o, d = R.axis(boxes(name), N_SMALL, 23)
        elif kind == "inside":
            o, d = R.inside(focus(name), N_SMALL, 24)
        else:
            o, d = R.away(boxes(name)[0], N_SMALL, 25)
        o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
        assert R.passes(o, d).all(), (name, kind)  # every generator ray passes the 2^-20 test
        o.setflags(write=False)
        d.setflags(write=False)
        _rays[name, kind] = (o, d)
    return _rays[name, kind]


def dev():
    return torch.device("cuda", 0)


def query(eng, orig, dirs, variant=E.ATR_KERNEL_AUTO, sort_bits=-1, stream=None, wait=True, **kw):
    """One atr_trace_rays call; numpy outputs (face as uint32) and the traced-ray count."""
    o = torch.from_numpy(np.array(orig, F)).to(dev())  # copies: the cached batches are read-only
    d = torch.from_numpy(np.array(dirs, F)).to(dev())
    out, traced = eng.trace_rays(o, d, variant=variant, sort_bits=sort_bits, stream=stream, **kw)
    if not wait:
        return out, traced, (o, d)
    rc, done = eng.wait()
    assert rc == 0 and done == 0, (rc, done)
    torch.cuda.synchronize()
    return host(out, traced)


def host(out, traced):
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if "face" in res:
        res["face"] = res["face"].view(np.uint32)
    res["traced"] = int(traced.item())
    return res


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_parity(res, want, what, rows=None):
    face, t, uv = (a if rows is None else a[rows] for a in want)
    got = res if rows is None else {k: (v[rows] if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    bad = np.flatnonzero(got["face"] != face)
    assert len(bad) == 0, (what, "face", len(bad), bad[:5].tolist())
    bad = np.flatnonzero(bits(got["t"]) != bits(t))
    assert len(bad) == 0, (what, "t", len(bad), bad[:5].tolist())
    bad = np.flatnonzero((bits(got["uv"]) != bits(uv)).any(axis=1))
    assert len(bad) == 0, (what, "uv", len(bad), bad[:5].tolist())


# ---- 1. parity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["aimed", "second", "axis", "inside", "away"])
@pytest.mark.parametrize("name", list(SCENES))
def test_parity_with_oracle(eng, name, kind):
    SCENES[name].upload(eng)
    orig, dirs = rays(name, kind)
    want = trace(name, orig, dirs, kind)
    if name != "nomodel" and kind in ("aimed", "second", "axis"):
        assert int((want[0] != R.MISS).sum()) >= 100, (name, kind)  # triangles are hit
    for variant in VARIANTS:
        for sb in SORTS:
            res = query(eng, orig, dirs, variant, sb)
            assert_parity(res, want, (name, kind, variant, sb))
            assert res["traced"] == len(orig), (name, kind, variant, sb, res["traced"])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_parity_at_wave_tails(eng, n):
    MIXED.upload(eng)
    orig, dirs = (a[:n] for a in rays("mixed", "aimed"))
    want = tuple(a[:n] for a in trace("mixed", *rays("mixed", "aimed"), "aimed"))
    for variant in VARIANTS:
        for sb in SORTS + (-1,):
            res = query(eng, orig, dirs, variant, sb)
            assert_parity(res, want, (n, variant, sb))
            assert res["traced"] == n


# ---- 2. model, kind, material ------------------------------------------------------------------------

def derived(name, orig, dirs):
    """kind, model and material from oracle traces only: the scene composed without spheres and
    planes (t_m), with the spheres only (t_ms) and in full (t_all), and its parts' own traces."""
    sc = SCENES[name]
    t_all = trace(name, orig, dirs)[1]
    face_all = trace(name, orig, dirs)[0]
    t_m = Sc(sc.names, sc.model_mats, sc.materials).oracle().trace(orig, dirs)[1]
    t_ms = Sc(sc.names, sc.model_mats, sc.materials, sc.spheres).oracle().trace(orig, dirs)[1]
    kind = np.where(t_all < t_ms, E.ATR_RAY_PLANE,
                    np.where(t_ms < t_m, E.ATR_RAY_SPHERE,
                             np.where(face_all != R.MISS, E.ATR_RAY_TRI, E.ATR_RAY_SKY))).astype(np.int32)
    best = np.full(len(orig), R.MAX_FLOAT, F)
    who = np.full(len(orig), -1, np.int32)
    for i, p in enumerate(sc.parts()):  # closest_of_singles' rule, applied to trace
        f, ti, _, _ = p.trace(orig, dirs)
        win = (f != R.MISS) & (ti < best)
        best[win], who[win] = ti[win], i
    model = np.where(kind == E.ATR_RAY_TRI, who, -1).astype(np.int32)
    assert len(sc.spheres) <= 1 and len(sc.planes) <= 1  # one candidate each: its material
    material = np.zeros(len(orig), np.int32)
    material[kind == E.ATR_RAY_TRI] = np.asarray(sc.model_mats, np.int32)[model[kind == E.ATR_RAY_TRI]]
    if sc.spheres:
        material[kind == E.ATR_RAY_SPHERE] = sc.spheres[0][2]
    if sc.planes:
        material[kind == E.ATR_RAY_PLANE] = sc.planes[0][2]
    return kind, model, material


def mixed_batch():
    o = np.concatenate([rays("mixed", k)[0] for k in ("aimed", "second", "away")])
    d = np.concatenate([rays("mixed", k)[1] for k in ("aimed", "second", "away")])
    return o, d


@pytest.mark.parametrize("name", ["mixed", "ties"])
def test_model_kind_material(eng, name):
    SCENES[name].upload(eng)
    orig, dirs = mixed_batch() if name == "mixed" else rays(name, "aimed")
    kind, model, material = derived(name, orig, dirs)
    if name == "mixed":
        assert set(np.unique(kind).tolist()) == {0, 1, 2, 3}  # sky, triangles, the sphere and the plane
        assert set(np.unique(model).tolist()) == {-1, 0, 1, 2, 3}  # and every model
    else:
        assert int((kind == E.ATR_RAY_TRI).sum()) >= 500
        assert (model[kind == E.ATR_RAY_TRI] == 0).all()  # coincident Monkeys: the first wins
    for variant in VARIANTS:
        for sb in (0, 5):
            res = query(eng, orig, dirs, variant, sb)
            for k, want in (("kind", kind), ("model", model), ("material", material)):
                bad = np.flatnonzero(res[k] != want)
                assert len(bad) == 0, (name, variant, sb, k, len(bad), bad[:5].tolist(), res[k][bad[:5]], want[bad[:5]])


# ---- 3. the normal -------------------------------------------------------------------------------------

def np_unit(v):
    return R.unit(v)


def np_cross(a, b):  # engine.h:51
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(F)


def shade_normal(sc, orig, dirs, res):
    """shade.h:51-78 restated in numpy float32, in its order of operations: the plane's own normal
    (:52-55), the sphere's (o + d * t) - centre (:57-60), a smooth model's interpolated vertex normals
    na * (1 - u - v) + nb * u + nc * v (:66-68), a flat model's cross(v0 - v1, v0 - v2) (:69-72); then
    unit() unless the ray met the sky (:78). Inputs: the engine's own kind, model, face, t and uv,
    each checked against the oracle by the tests above."""
    n = np.zeros((len(orig), 3), F)
    kind, model, face, t, uv = res["kind"], res["model"], res["face"], res["t"], res["uv"]
    pl = kind == E.ATR_RAY_PLANE
    if pl.any():
        n[pl] = np.asarray(sc.planes[0][0], F)
    sp = kind == E.ATR_RAY_SPHERE
    if sp.any():
        n[sp] = (orig[sp] + dirs[sp] * t[sp][:, None]) - np.asarray(sc.spheres[0][0], F)
    for i, p in enumerate(sc.parts()):
        m = (kind == E.ATR_RAY_TRI) & (model == i)
        if not m.any():
            continue
        V, N, FV, FN = p.mesh_arrays()
        f = face[m].astype(np.int64)
        if len(N):  # smooth
            na, nb, nc = (N[FN[f, k]] for k in range(3))
            u, v = uv[m, 0], uv[m, 1]
            w = (F(1.0) - u) - v
            n[m] = (na * w[:, None] + nb * u[:, None]) + nc * v[:, None]
        else:  # flat
            v0, v1, v2 = (V[FV[f, k]] for k in range(3))
            n[m] = np_cross(v0 - v1, v0 - v2)
    hit = kind != E.ATR_RAY_SKY
    n[hit] = np_unit(n[hit])
    return n


def test_normal_matches_shade_h(eng):
    MIXED.upload(eng)
    orig, dirs = mixed_batch()
    for variant in VARIANTS:
        res = query(eng, orig, dirs, variant, 5)
        want = shade_normal(MIXED, orig, dirs, res)
        tri = res["kind"] == E.ATR_RAY_TRI
        assert int((tri & (res["model"] == 1)).sum()) >= 100  # the Monkey: smooth
        assert int((tri & (res["model"] == 2)).sum()) >= 100  # the Deer: flat
        assert int((res["kind"] == E.ATR_RAY_SPHERE).sum()) >= 20 and int((res["kind"] == E.ATR_RAY_PLANE).sum()) >= 20
        bad = np.flatnonzero((bits(res["normal"]) != bits(want)).any(axis=1))
        assert len(bad) == 0, (variant, len(bad), bad[:5].tolist(), res["kind"][bad[:5]], res["normal"][bad[:5]],
                               want[bad[:5]])
        assert (res["normal"][res["kind"] == E.ATR_RAY_SKY] == 0).all()


# ---- 4. invalid rays -------------------------------------------------------------------------------------

def invalid_batch():
    """320 aimed Monkey-scene rays; rows 64..127 (a whole wavefront in input order) and a few more are
    made invalid, and two rays sit exactly on the validity bound (len2 - 1 = +-2^-20: valid)."""
    orig, dirs = (a[:320].copy() for a in rays("mixed", "aimed"))
    bad = np.zeros(320, bool)
    nan, inf = F(np.nan), F(np.inf)
    edits = [(3, "d", lambda d: d * F(0.5)), (4, "d", lambda d: d * F(2.0)), (5, "d", lambda d: d * F(0.0)),
             (6, "d", lambda d: np.array([nan, d[1], d[2]], F)), (7, "d", lambda d: np.array([d[0], inf, d[2]], F)),
             (8, "o", lambda o: np.array([o[0], o[1], nan], F)), (9, "o", lambda o: np.array([-inf, o[1], o[2]], F)),
             (10, "d", lambda d: np.array([1 + 2.0 ** -20, 0, 0], F)), (11, "d", lambda d: np.array([0, 1 - 2.0 ** -20, 0], F)),
             (319, "d", lambda d: np.array([nan, nan, nan], F))]
    for row, which, fn in edits:
        a = orig if which == "o" else dirs
        a[row] = fn(a[row])
        bad[row] = True
    dirs[64:128] *= F(1.5)
    bad[64:128] = True
    monkey = np.asarray(boxes("mixed")[2], F)
    ctr = (monkey[:3] + monkey[3:]) * F(0.5)
    orig[12] = ctr - np.array([5, 0, 0], F)
    dirs[12] = np.array([1 + 2.0 ** -21, 0, 0], F)  # len2 = 1 + 2^-20
    orig[13] = ctr + np.array([0, 5, 0], F)
    dirs[13] = np.array([0, -(1 - 2.0 ** -21), 0], F)  # len2 = 1 - 2^-20
    ok = R.passes(orig, dirs)
    assert np.array_equal(ok, ~bad)
    return orig, dirs, ok


def test_invalid_rays_are_not_traced(eng):
    MIXED.upload(eng)
    orig, dirs, ok = invalid_batch()
    want = tuple(a for a in SCENES["mixed"].oracle().trace(orig[ok], dirs[ok])[:3])
    edge = [list(np.flatnonzero(ok)).index(r) for r in (12, 13)]  # the two rays on the validity bound
    assert (want[1][edge] < R.MAX_FLOAT).all() and want[0][edge[0]] != R.MISS  # hit something; one a triangle
    for variant in VARIANTS:
        for sb in SORTS:
            res = query(eng, orig, dirs, variant, sb)
            what = (variant, sb)
            assert (res["kind"][~ok] == E.ATR_RAY_INVALID).all(), what
            assert (res["kind"][ok] != E.ATR_RAY_INVALID).all(), what
            assert (bits(res["t"][~ok]) == bits(R.MAX_FLOAT)).all() and (res["face"][~ok] == R.MISS).all(), what
            assert (res["model"][~ok] == -1).all() and (res["material"][~ok] == 0).all(), what
            assert (bits(res["uv"][~ok]) == 0).all() and (bits(res["normal"][~ok]) == 0).all(), what
            assert_parity({k: (v[ok] if isinstance(v, np.ndarray) else v) for k, v in res.items()}, want, what)
            assert res["traced"] == int(ok.sum()), (what, res["traced"])


# ---- 5. independence of order ------------------------------------------------------------------------------

def test_results_do_not_depend_on_batch_order(eng):
    MIXED.upload(eng)
    orig, dirs = mixed_batch()
    perm = np.random.default_rng(31).permutation(len(orig))
    for sb in SORTS:
        a = query(eng, orig, dirs, E.ATR_KERNEL_AUTO, sb)
        b = query(eng, orig[perm], dirs[perm], E.ATR_KERNEL_AUTO, sb)
        for k in ("t", "face", "model", "uv", "kind", "material", "normal"):
            assert np.array_equal(np.ascontiguousarray(a[k][perm]).view(np.uint32),
                                  np.ascontiguousarray(b[k]).view(np.uint32)), (sb, k)
        assert a["traced"] == b["traced"] == len(orig)


# ---- 6. partial outputs and streams ---------------------------------------------------------------------------

def raw_call(eng, o, d, n, hits, variant=E.ATR_KERNEL_AUTO, sort_bits=0, stream=None):
    return E.lib().atr_trace_rays(eng.h, C.c_void_p(o.data_ptr()) if o is not None else None,
                                  C.c_void_p(d.data_ptr()) if d is not None else None, n,
                                  C.byref(hits) if hits is not None else None, variant, sort_bits,
                                  C.c_void_p(stream) if stream else None)


def test_only_the_requested_output_is_written(eng):
    MIXED.upload(eng)
    orig, dirs = rays("mixed", "aimed")
    n = len(orig)
    o, d = torch.from_numpy(orig.copy()).to(dev()), torch.from_numpy(dirs.copy()).to(dev())
    buf = torch.full((3 * n,), -7.0, dtype=torch.float32, device=dev())
    hits = E.atr_ray_hits(t=buf.data_ptr() + 4 * n)
    for sb in (0, 5):
        buf.fill_(-7.0)
        assert raw_call(eng, o, d, n, hits, sort_bits=sb, stream=torch.cuda.current_stream().cuda_stream) == 0
        assert eng.wait() == (0, 0)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[:n] == -7.0).all() and (got[2 * n:] == -7.0).all()
        assert np.array_equal(bits(got[n:2 * n]), bits(trace("mixed", orig, dirs, "aimed")[1]))
    res = query(eng, orig, dirs, outputs=("t", "kind"))
    assert sorted(res) == ["kind", "t", "traced"]


def test_two_streams_with_a_render_between(eng):
    MIXED.upload(eng)
    W, H = 96, 72
    s1, s2 = torch.cuda.Stream(dev()), torch.cuda.Stream(dev())
    a, b = rays("mixed", "aimed"), rays("mixed", "second")
    torch.cuda.synchronize()
    ra = query(eng, *a, sort_bits=5, stream=s1.cuda_stream, wait=False)
    assert eng.wait()[0] == 0 and eng.last_kernel_ms() > 0
    r = run(eng, E.camera(W, H, 2, 3))
    rb = query(eng, *b, sort_bits=5, stream=s2.cuda_stream, wait=False)
    assert eng.wait()[0] == 0 and eng.last_kernel_ms() > 0
    torch.cuda.synchronize()
    assert_parity(host(*ra[:2]), trace("mixed", *a, "aimed"), "stream 1")
    assert_parity(host(*rb[:2]), trace("mixed", *b, "second"), "stream 2")
    want = ref(MIXED, W, H, 2, 3)
    assert np.array_equal(r["fb"], want["fb"]) and np.array_equal(r["casts"], want["casts"])
    # back to back on two streams without a wait between: the shared workspace is handed over on the GPU
    ra = query(eng, *a, sort_bits=5, stream=s1.cuda_stream, wait=False)
    rb = query(eng, *b, sort_bits=2, stream=s2.cuda_stream, wait=False)
    assert eng.wait()[0] == 0
    torch.cuda.synchronize()
    assert_parity(host(*ra[:2]), trace("mixed", *a, "aimed"), "stream 1 again")
    assert_parity(host(*rb[:2]), trace("mixed", *b, "second"), "stream 2 again")


# ---- 7. arguments ---------------------------------------------------------------------------------------------

def test_arguments(eng):
    MIXED.upload(eng)
    orig, dirs = (a[:65] for a in rays("mixed", "aimed"))
    n = 65
    o, d = torch.from_numpy(np.array(orig, F)).to(dev()), torch.from_numpy(np.array(dirs, F)).to(dev())
    t = torch.full((n,), -7.0, dtype=torch.float32, device=dev())
    traced = torch.full((1,), 5, dtype=torch.int64, device=dev())
    hits = E.atr_ray_hits(t=t.data_ptr(), traced_rays=traced.data_ptr())
    inv = -1
    assert raw_call(eng, o, d, n, None) == inv
    assert raw_call(eng, None, d, n, hits) == inv
    assert raw_call(eng, o, None, n, hits) == inv
    assert raw_call(eng, o, d, -1, hits) == inv
    assert raw_call(eng, o, d, 2 ** 31, hits) == inv
    for variant in (E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_PATHS, 2, -1):
        assert raw_call(eng, o, d, n, hits, variant=variant) == inv
    for sb in (1, 8, -2, 64):
        assert raw_call(eng, o, d, n, hits, sort_bits=sb) == inv
    assert raw_call(eng, o, d, 0, hits) == 0 and raw_call(eng, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert (t.cpu().numpy() == -7.0).all() and int(traced.item()) == 5  # nothing was written
    for variant in (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_FLAT, E.ATR_KERNEL_LANE):
        for sb in (-1, 0, 2, 7):
            assert raw_call(eng, o, d, n, hits, variant=variant, sort_bits=sb,
                            stream=torch.cuda.current_stream().cuda_stream) == 0
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    assert int(traced.item()) == 5 + 12 * n  # one accumulator, added to
    assert np.array_equal(bits(t.cpu().numpy()), bits(trace("mixed", *rays("mixed", "aimed"), "aimed")[1][:n]))
    with pytest.raises(ValueError):
        eng.trace_rays(o.t().contiguous().t(), d)  # not contiguous
    with pytest.raises(ValueError):
        eng.trace_rays(o.double(), d)
    fresh = E.Engine(0)
    try:
        assert raw_call(fresh, o, d, n, hits) == -4  # ATR_E_NOSCENE
    finally:
        fresh.close()


# ---- 8. growth ---------------------------------------------------------------------------------------------------

def test_workspace_growth(eng):
    orig, dirs = rays("mixed", "aimed")
    want = trace("mixed", orig, dirs, "aimed")
    a, b = E.Engine(0), E.Engine(0)
    try:
        for e in (a, b):
            MIXED.upload(e)
        ws0 = a.workspace_info()
        small = query(a, orig[:64], dirs[:64], sort_bits=2)
        assert_parity(small, tuple(x[:64] for x in want), "64 rays")
        grown = query(a, orig, dirs, sort_bits=5)  # more rays and more bins than the workspace holds
        fresh = query(b, orig, dirs, sort_bits=5)
        for k in ("t", "face", "model", "uv", "kind", "material", "normal"):
            assert np.array_equal(np.ascontiguousarray(grown[k]).view(np.uint32),
                                  np.ascontiguousarray(fresh[k]).view(np.uint32)), k
        assert_parity(grown, want, "4097 rays after 64")
        again = query(a, orig[:64], dirs[:64], sort_bits=2)  # and a small batch in the grown workspace
        assert_parity(again, tuple(x[:64] for x in want), "64 rays again")
        assert a.workspace_info() == ws0  # the path workspaces' report is what it was
    finally:
        a.close()
        b.close()
