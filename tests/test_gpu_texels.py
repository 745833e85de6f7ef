"""atr_mesh_texels and atr_texels_to_image on the GPU: every output for exact equality with the plain C
reference of tests/texel_ref.py (pinned without a GPU in tests/test_texels_cpu.py): the loader's meshes
and a jittered UV grid at sizes that take the in-lane path, the listed-face path (a 12-face cube on a
2,048 x 2,048 map) and every level of the slot scan; the size query; the image call on a stream of its
own; a bake end to end against the composed references; the arguments; a render before and after.
Every buffer is filled with a sentinel first and guarded on both sides. Needs an MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import gather_radiance_ref as GRR  # noqa: E402
from tests import gather_ref as GR  # noqa: E402
from tests import texel_ref as TX  # noqa: E402
from tests.test_gpu_parity import eng, run  # noqa: E402,F401
from tests.test_texels_cpu import grid_obj  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
G = 256  # guard bytes around every output buffer
FILL = 0xAB
PER = {"slot": 4, "texel": 4, "face": 4, "bary": 8, "point": 12, "normal": 12}  # bytes per element
SEED = 0x853C49E6748FEA9B

_meshes = {}


def mesh(name):
    """(Mesh, Mesh.arrays()) of a golden asset or of the n = 20 grid, cached."""
    if name not in _meshes:
        m = E.Mesh.parse_obj(grid_obj(20, 512, 512)) if name == "grid20" else E.Mesh.load_obj(asset_path(name))
        _meshes[name] = (m, m.arrays())
    return _meshes[name]


def dev():
    return torch.device("cuda", 0)


class Bufs:
    """slot for `ntexels` and the per-k outputs for `cap` elements, 0xAB-filled with guards."""

    def __init__(self, ntexels, cap, names=TX.KEYS):
        self.count = {k: ntexels if k == "slot" else cap for k in TX.KEYS}
        self.names = names
        self.buf = {k: torch.full((self.count[k] * PER[k] + 2 * G,), FILL, dtype=torch.uint8, device=dev())
                    for k in names}

    def out(self):
        return E.atr_texels_out(*[self.buf[k].data_ptr() + G if k in self.names else None for k in TX.KEYS])

    def raw(self, k):
        a = self.buf[k].cpu().numpy()
        n = self.count[k] * PER[k]
        assert (a[:G] == FILL).all() and (a[G + n:] == FILL).all(), (k, "guard bytes")
        return a[G:G + n].copy()

    def get(self, k, n=None):
        a = self.raw(k)
        a = a.view(F) if k in ("bary", "point", "normal") else a.view(np.uint32 if k == "face" else np.int32)
        a = a.reshape(-1, PER[k] // 4) if PER[k] > 4 else a
        return a if n is None or k == "slot" else a[:n]


def call(eng, m, w, h, bufs, cap, flags=0, ms=None):
    n = C.c_int64(-5)
    torch.cuda.synchronize()  # the fills above, ahead of a call on the context's own stream
    rc = E.lib().atr_mesh_texels(eng.h, m.h, w, h, flags, cap, C.byref(bufs.out()) if bufs is not None else None,
                                 C.byref(n), ms)
    return rc, n.value


def check_all(eng, name, w, h, flip=False):
    m, arr = mesh(name)
    ref = TX.mesh_texels(arr, w, h, flip=flip)
    k = len(ref["texel"])
    b = Bufs(w * h, k)
    ms = (C.c_float * 2)()
    rc, n = call(eng, m, w, h, b, k, flags=E.ATR_TEXELS_FLIP if flip else 0, ms=ms)
    assert rc == 0 and n == k, (rc, n, k)
    assert ms[0] > 0 and 0 < ms[1] <= ms[0]
    for key in TX.KEYS:
        assert TX.same_bits(b.get(key, k), ref[key]), (name, w, h, key)
    return ref


# Cube and Deer at the reference's sizes; the grid at 512 x 512 (800 faces of ~330 texels: the list);
# Cube at 2,048 x 2,048 (12 faces over 4 M texels: the listed faces' tiles, and 4,096 scan blocks, 4 per
# thread of the second level); Deer at 1,024 x 1,025: 1,026 scan blocks, the smallest count above the
# second level's 1,024 threads with a ragged last thread (a block holds 1,024 texels, so every size of
# more than 1,024 texels crosses the first level).
@pytest.mark.parametrize("name,w,h", [(a, w, h) for a in ("Cube", "Deer") for w, h in [(1, 1), (7, 5), (64, 64), (200, 120)]]
                         + [("grid20", 512, 512), ("Cube", 2048, 2048), ("Deer", 1024, 1025)])
def test_outputs_equal_the_reference(eng, name, w, h):  # noqa: F811
    ref = check_all(eng, name, w, h)
    t = ref["texel"]
    assert (np.diff(t.astype(np.int64)) > 0).all() and np.array_equal(ref["slot"][t], np.arange(len(t)))
    if name == "grid20":
        assert len(t) == w * h  # watertight on the device too


def test_flip_and_partial_outputs(eng):  # noqa: F811
    check_all(eng, "Cube", 64, 64, flip=True)
    check_all(eng, "Deer", 200, 120, flip=True)
    m, arr = mesh("Deer")
    ref = TX.mesh_texels(arr, 64, 64)
    k = len(ref["texel"])
    for names in [("point", "normal"), ("slot",), ("texel",), ("bary", "face")]:
        b = Bufs(64 * 64, k, names)
        rc, n = call(eng, m, 64, 64, b, k)
        assert rc == 0 and n == k
        for key in names:
            assert TX.same_bits(b.get(key, k), ref[key]), (names, key)


def test_size_query_leaves_the_arrays_alone(eng):  # noqa: F811
    m, arr = mesh("Deer")
    w, h = 200, 120
    ref = TX.mesh_texels(arr, w, h)
    k = len(ref["texel"])
    for cap in (k - 1, 0):
        b = Bufs(w * h, k)
        rc, n = call(eng, m, w, h, b, cap)
        assert rc == 0 and n == k
        assert np.array_equal(b.get("slot"), ref["slot"])
        for key in TX.KEYS[1:]:
            assert (b.raw(key) == FILL).all(), key
    # a larger cap than needed is fine: the tail stays untouched
    b = Bufs(w * h, k + 3)
    rc, n = call(eng, m, w, h, b, k + 3)
    assert rc == 0 and n == k
    assert TX.same_bits(b.get("point", k), ref["point"]) and (b.raw("point")[12 * k:] == FILL).all()


def test_engine_mesh_texels(eng):  # noqa: F811
    m, arr = mesh("Cube")
    ref = TX.mesh_texels(arr, 200, 120)
    tm = {}
    got = eng.mesh_texels(m, 200, 120, timings=tm)
    assert sorted(got) == sorted(TX.KEYS) and tm["device_ms"] > 0
    for key in TX.KEYS:
        assert TX.same_bits(got[key].cpu().numpy(), ref[key]), key
    t, slot = got["texel"].cpu().numpy(), got["slot"].cpu().numpy()
    assert (np.diff(t) > 0).all() and np.array_equal(slot[t], np.arange(len(t)))
    empty = eng.mesh_texels(m, 1, 1)  # the Cube's layout leaves the only centre uncovered
    assert empty["texel"].numel() == 0 and empty["slot"].cpu().numpy().tolist() == [-1]


def test_arguments(eng):  # noqa: F811
    m, _ = mesh("Cube")
    bare = E.Mesh.parse_obj("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")  # no texcoords
    n = C.c_int64()
    out = E.atr_texels_out()
    f = E.lib().atr_mesh_texels
    bad = E.ERRORS
    assert bad[f(None, m.h, 8, 8, 0, 0, C.byref(out), C.byref(n), None)] == "ATR_E_INVALID"
    assert bad[f(eng.h, None, 8, 8, 0, 0, C.byref(out), C.byref(n), None)] == "ATR_E_INVALID"
    assert bad[f(eng.h, m.h, 8, 8, 0, 0, None, C.byref(n), None)] == "ATR_E_INVALID"
    assert bad[f(eng.h, m.h, 8, 8, 0, 0, C.byref(out), None, None)] == "ATR_E_INVALID"
    assert bad[f(eng.h, bare.h, 8, 8, 0, 0, C.byref(out), C.byref(n), None)] == "ATR_E_INVALID"
    for w, h in [(0, 8), (8, 0), (-1, 8), (16385, 8), (8, 16385)]:
        assert bad[f(eng.h, m.h, w, h, 0, 0, C.byref(out), C.byref(n), None)] == "ATR_E_INVALID"
    assert bad[f(eng.h, m.h, 8, 8, 0, -1, C.byref(out), C.byref(n), None)] == "ATR_E_INVALID"
    assert bad[f(eng.h, m.h, 8, 8, 2, 0, C.byref(out), C.byref(n), None)] == "ATR_E_INVALID"
    assert f(eng.h, m.h, 16384, 1, 0, 0, C.byref(out), C.byref(n), None) == 0  # all outputs NULL: the count alone
    g = E.lib().atr_texels_to_image
    img = torch.zeros(8 * 8 * 3, dtype=torch.float32, device=dev())
    val = torch.zeros(3 * 3, dtype=torch.float32, device=dev())
    tex = torch.zeros(3, dtype=torch.int32, device=dev())
    fill = (C.c_float * 3)(0, 0, 0)
    p = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    assert bad[g(None, p(val), p(tex), 3, 8, 8, 1, fill, p(img), None)] == "ATR_E_INVALID"
    assert bad[g(eng.h, p(val), p(tex), 3, 8, 8, 1, fill, None, None)] == "ATR_E_INVALID"
    assert bad[g(eng.h, None, p(tex), 3, 8, 8, 1, fill, p(img), None)] == "ATR_E_INVALID"
    assert bad[g(eng.h, p(val), None, 3, 8, 8, 1, fill, p(img), None)] == "ATR_E_INVALID"
    assert bad[g(eng.h, p(val), p(tex), -1, 8, 8, 1, fill, p(img), None)] == "ATR_E_INVALID"
    assert bad[g(eng.h, p(val), p(tex), 65, 8, 8, 1, fill, p(img), None)] == "ATR_E_INVALID"
    assert bad[g(eng.h, p(val), p(tex), 3, 0, 8, 1, fill, p(img), None)] == "ATR_E_INVALID"
    assert bad[g(eng.h, p(val), p(tex), 3, 8, 16385, 1, fill, p(img), None)] == "ATR_E_INVALID"
    assert bad[g(eng.h, p(val), p(tex), 3, 8, 8, -1, fill, p(img), None)] == "ATR_E_INVALID"
    assert bad[g(eng.h, p(val), p(tex), 3, 8, 8, 65, fill, p(img), None)] == "ATR_E_INVALID"
    assert (img == 0).all()


@pytest.mark.parametrize("w,h", [(7, 5), (200, 120)])
def test_image_equals_the_reference_on_its_own_stream(eng, w, h):  # noqa: F811
    _, arr = mesh("Cube")
    texel = TX.mesh_texels(arr, w, h)["texel"]
    vals = np.random.default_rng(w).uniform(-2, 5, (len(texel), 3)).astype(F)
    tv, tt = torch.from_numpy(vals).to(dev()), torch.from_numpy(texel).to(dev())
    fill = (0.25, -1.0, 7.0)
    st = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    for passes in (0, 1, 2, 64):
        buf = torch.full((w * h * 12 + 2 * G,), FILL, dtype=torch.uint8, device=dev())
        torch.cuda.synchronize()
        rc = E.lib().atr_texels_to_image(eng.h, C.c_void_p(tv.data_ptr()), C.c_void_p(tt.data_ptr()), len(texel), w, h,
                                         passes, (C.c_float * 3)(*fill), C.c_void_p(buf.data_ptr() + G),
                                         C.c_void_p(st.cuda_stream))
        assert rc == 0
        rc, done = eng.wait()
        assert rc == 0 and done == 0
        a = buf.cpu().numpy()
        assert (a[:G] == FILL).all() and (a[-G:] == FILL).all()
        want = TX.texels_to_image(vals, texel, w, h, passes, fill)
        assert TX.same_bits(a[G:-G].view(F).reshape(h, w, 3), want), passes
    # the Engine method, on torch's current stream, right behind a call on the other stream
    got = eng.texels_to_image(tv, tt, w, h, passes=2, fill=fill)
    rc, _ = eng.wait()
    assert rc == 0
    assert TX.same_bits(got.cpu().numpy(), TX.texels_to_image(vals, texel, w, h, 2, fill))


def test_bake_equals_the_composed_references(eng):  # noqa: F811
    """The Cube with a sphere above it, 64 x 64 texels, 16 samples: texels, gather, image on the device
    against texel_ref, the gathers' references on the reference's points, and the dilation reference."""
    w = h = 64
    ns = 16
    m = E.Mesh.load_obj(asset_path("Cube"))
    box = m.translate_to(m.aabb(), CENTERS["Cube"])
    cx, cy, cz = CENTERS["Cube"]
    spheres = [((cx + 0.3, cy + 1.6, cz), 0.9, 2)]
    mats = [O.SKY, O.MODEL_MAT, ((0.9, 0.7, 0.3), (0.6, 0.6, 0.6), 0.8)]
    eng.upload(mats, [(m, E.Octree.build(m, 300), box, 1)], spheres)
    scene = O.Scene(asset_path("Cube"), center=CENTERS["Cube"], materials=mats, spheres=spheres)
    tex = TX.mesh_texels(m.arrays(), w, h)
    k = len(tex["texel"])
    assert k == 2709
    # visibility
    g = GR.gather(scene, tex["point"], tex["normal"], ns, seed=SEED)
    vis, tot = g["visible"].astype(F), (g["visible"] + g["occluded"]).astype(F)
    assert (tot > 0).all() and 0 < (g["occluded"] > 0).sum() < k  # the sphere shadows some texels, not all
    val = np.where(tot > 0, vis / np.maximum(tot, F(1)), F(0)).astype(F)
    want = TX.texels_to_image(np.repeat(val[:, None], 3, 1), tex["texel"], w, h, 2)
    img, got = eng.bake_lightmap(m, w, h, ns, seed=SEED)
    for key in TX.KEYS:
        assert TX.same_bits(got[key].cpu().numpy(), tex[key]), key
    assert TX.same_bits(img.cpu().numpy(), want)
    # radiance, two bounces
    r = GRR.gather_radiance(scene, tex["point"], tex["normal"], ns, 2, seed=SEED)
    assert (r["invalid"] == 0).all()
    want = TX.texels_to_image(r["rgb"], tex["texel"], w, h, 2)
    img, _ = eng.bake_lightmap(m, w, h, ns, bounces=2, seed=SEED)
    assert TX.same_bits(img.cpu().numpy(), want)
    assert len(np.unique(img.cpu().numpy().reshape(-1, 3), axis=0)) > 100


def test_render_unchanged_by_the_texel_calls(eng):  # noqa: F811
    m = E.Mesh.load_obj(asset_path("Deer"))
    box = m.translate_to(m.aabb(), CENTERS["Deer"])
    eng.upload([O.SKY, O.MODEL_MAT], [(m, E.Octree.build(m, 300), box, 1)])
    cam = E.camera(96, 54, 2, 3)
    before = run(eng, cam)
    img, _ = eng.bake_lightmap(m, 200, 120, 4)
    eng.bake_lightmap(m, 64, 64, 4, bounces=2)
    assert torch.isfinite(img).all()
    after = run(eng, cam)
    assert (before["face"] != E.MISS).any()
    for key in ("fb", "face", "t", "rgb", "casts"):
        assert np.array_equal(before[key].view(np.uint32), after[key].view(np.uint32)), key
    assert before["traced"] == after["traced"]
