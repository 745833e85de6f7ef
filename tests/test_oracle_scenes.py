"""The composed (several-model) oracle, ``oracle.Scene.compose``, against something other than its
own model loop: the closest hit over the parts' one-model scenes, the framebuffer recomputed on the
host from that winner's material, and the first-model-wins rule on two coincident meshes. CPU only."""
import numpy as np

from atray_amd.assets import CENTERS, asset_path
from oracle import oracle as O

M = 0xFFFFFFFF
W, H = 96, 72
# a distinct emission per model, no component above 1 (the clamp is then the identity)
MATS = [O.SKY, ((0.9, 0.1, 0.2), (0.5, 0.5, 0.5), 0.3), ((0.1, 0.8, 0.3), (0.5, 0.5, 0.5), 0.3),
        ((0.2, 0.3, 0.95), (0.5, 0.5, 0.5), 0.3)]

_parts = {}


def part(asset, leaf, material, tree=True, center=None):
    key = (asset, leaf, material, tree, center)
    if key not in _parts:
        _parts[key] = O.Scene(asset_path(asset), center=center or CENTERS[asset], max_faces=leaf, use_tree=tree,
                              model_material=material)
    return _parts[key]


def three():
    return [part("Cube", 300, 1), part("Monkey", 64, 2), part("Deer", 300, 3)]


def closest_of_singles(parts, cam):
    """(face, t, winning model or -1) per pixel from the parts' own one-model primary hits: the
    smallest t, the lowest model index on equal t."""
    face = np.full((cam.height, cam.width), M, np.uint32)
    t = np.full((cam.height, cam.width), np.float32(3.402823466e38), np.float32)
    who = np.full((cam.height, cam.width), -1, np.int32)
    for i, p in enumerate(parts):
        f, ti, _ = p.primary_hits(cam)
        win = (f != M) & (ti < t)
        face[win], t[win], who[win] = f[win], ti[win], i
    return face, t, who


def emission_fb(who, materials, model_material):
    """The framebuffer of a 1-spp, 1-bounce render: the hit material's emission (material 0 for the
    sky), clamped to [0, 1], times 255 in f32, truncated, as BGRX."""
    mat = np.where(who >= 0, np.asarray(model_material, np.int32)[np.maximum(who, 0)], 0)
    em = np.asarray([m[0] for m in materials], np.float32)[mat]
    q = (np.clip(em, np.float32(0), np.float32(1)) * np.float32(255.0)).astype(np.int32).astype(np.uint32) & 0xFF
    return q[..., 2] | (q[..., 1] << 8) | (q[..., 0] << 16)


def test_one_node_cube_tree():
    st = part("Cube", 300, 1).tree_stats()
    assert st["nodes"] == 1 and st["leaves"] == 1  # the root is a leaf


def test_composed_hits_are_the_closest_of_the_singles():
    parts = three()
    cam = O.Camera(W, H)
    f, t, _ = O.Scene.compose(parts, MATS).primary_hits(cam)
    wf, wt, who = closest_of_singles(parts, cam)
    assert np.array_equal(f, wf)
    assert np.array_equal(t.view(np.uint32), wt.view(np.uint32))
    wins = [int((who == i).sum()) for i in range(3)]
    assert min(wins) >= 50, wins  # every model is in view


def test_composed_render_shows_which_model_was_hit():
    parts = three()
    cam = O.Camera(W, H)
    _, _, who = closest_of_singles(parts, cam)
    rgb, fb, casts, _ = O.Scene.compose(parts, MATS).render(O.Camera(W, H, spp=1, bounces=1), 7)
    assert np.array_equal(fb, emission_fb(who, MATS, [1, 2, 3]))
    assert len(np.unique(fb)) == 4  # the sky and three models
    assert np.array_equal(casts, (who >= 0).astype(np.uint32))


def test_first_model_wins_a_tie():
    a, b = part("Monkey", 64, 1), part("Monkey", 64, 2)
    cam = O.Camera(W, H, spp=1, bounces=1)
    hit = a.primary_hits(O.Camera(W, H))[0] != M
    assert hit.sum() > 500
    for order, first in (([a, b], 1), ([b, a], 2)):
        _, fb, _, _ = O.Scene.compose(order, MATS).render(cam, 7)
        who = np.where(hit, 0, -1)
        assert np.array_equal(fb, emission_fb(who, MATS, [first, 3 - first]))
    ab = O.Scene.compose([a, b], MATS).render(cam, 7)[1]
    ba = O.Scene.compose([b, a], MATS).render(cam, 7)[1]
    assert np.array_equal(ab != ba, hit)  # the order flips the hit pixels and only those


def test_compose_keeps_its_parts_alive_and_the_single_scene_unchanged():
    p = O.Scene(asset_path("Cube"), center=CENTERS["Cube"])
    cam = O.Camera(48, 36)
    want = p.primary_hits(cam)
    s = O.Scene.compose([p], [O.SKY, O.MODEL_MAT])
    del p
    import gc
    gc.collect()
    got = s.primary_hits(cam)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert got[2] == want[2]
    assert (want[0] != M).sum() > 50
