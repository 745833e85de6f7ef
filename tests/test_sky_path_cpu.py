"""The sky path's record (engine.h SkyRecord), host side, no GPU: what atr_scene_upload
hands the primary kernels for the waves that read nothing of the scene must be the bits the slow path
would load -- a tree model's nodes[0] bounds (the tree's exported root), a brute-force model's
surrounding_aabb as given -- and the sky pixel that shade.h scene_finish leaves: material 0's emission,
face 0xFFFFFFFF, t = kMaxFloat. The path is off with more than four models or any sphere or plane.
atr_sky_record_host builds the record with the function the upload uses (capi.cpp sky_record)."""
import os
import re

import numpy as np
import pytest

from atray_amd import engine as E
from atray_amd.assets import CENTERS, asset_path
from oracle import oracle as O

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "atray_amd", "csrc")
SKY = ((0.3, -0.0, 1e-40), (0.2, 0.3, 0.4), 0.3)  # a negative zero and a denormal: the bits go through
MATS = [SKY, O.MODEL_MAT]
_parts = {}


def part(asset, leaf=300, tree=True, center=None):
    key = (asset, leaf, tree, center)
    if key not in _parts:
        m = E.Mesh.load_obj(asset_path(asset))
        box = m.translate_to(m.aabb(), center or CENTERS[asset])
        _parts[key] = (m, E.Octree.build(m, leaf) if tree else None, box, 1)
    return _parts[key]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def root_bounds(tree):
    return tree.export()[0][0]


def test_the_sky_pixel_is_scene_finish_s():
    """The constants, read from the sources the kernels are built from."""
    shade = open(os.path.join(CSRC, "shade.h")).read()
    fin = shade[shade.index("void scene_finish"):]
    assert re.search(r"id\.t = best;\s*id\.face = 0x([0-9A-Fa-f]+)u;", fin).group(1).upper() == "FFFFFFFF"
    sky = re.search(r"\} else \{\s*id\.type = T_SKY;\s*id\.material = (\d+);\s*\}", fin)
    assert sky and int(sky.group(1)) == 0  # no plane, no sphere, no model: the sky, material 0
    scan = open(os.path.join(CSRC, "scan.h")).read()
    assert re.search(r"SceneHit sh\{kMaxFloat,", scan)  # `best` of a ray that hits no model
    eng = open(os.path.join(CSRC, "engine.h")).read()
    assert re.search(r"kMaxFloat = 3\.402823466e\+38F", eng) and re.search(r"kSkyFace = 0xFFFFFFFFu", eng)
    assert int(re.search(r"kSkyBoxes = (\d+)", eng).group(1)) == 4
    r = E.sky_record(MATS, [part("Cube")])
    assert r["face"] == 0xFFFFFFFF == E.MISS
    assert bits(r["t"])[0] == 0x7F7FFFFF == bits([E.MAX_FLOAT])[0]
    assert np.array_equal(bits(r["emission"]), bits(SKY[0]))
    assert bits(r["emission"])[1] == 0x80000000 and 0 < bits(r["emission"])[2] < 0x00800000


@pytest.mark.parametrize("asset,leaf", [("Cube", 300), ("Cube", 6), ("Monkey", 64), ("Deer", 300)])
def test_a_tree_model_records_its_root_node(asset, leaf):
    p = part(asset, leaf)
    r = E.sky_record(MATS, [p])
    assert (r["on"], r["n"], r["brute"]) == (1, 1, 0)
    assert np.array_equal(bits(r["boxes"][0]), bits(root_bounds(p[1])))
    assert not r["boxes"][1:].any()


def test_a_brute_force_model_records_its_aabb_as_given():
    m, _, box, mat = part("Monkey", tree=False)
    odd = np.array(box, np.float32) + np.float32(0.125)  # not the mesh's bounds: the upload takes it as given
    r = E.sky_record(MATS, [(m, None, odd, mat)])
    assert (r["on"], r["n"], r["brute"]) == (1, 1, 1)
    assert np.array_equal(bits(r["boxes"][0]), bits(odd))


def test_four_models_in_order_five_switch_it_off():
    cubes = [part("Cube", center=(float(k), 0.5, -3.0 - k)) for k in range(5)]
    four = [cubes[0], part("Monkey", tree=False), cubes[1], part("Cube", tree=False, center=(1.3, 0.5, -3.2))]
    r = E.sky_record(MATS, four)
    assert (r["on"], r["n"], r["brute"]) == (1, 4, 0b1010)
    for k, p in enumerate(four):
        want = root_bounds(p[1]) if p[1] is not None else np.array(p[2], np.float32)
        assert np.array_equal(bits(r["boxes"][k]), bits(want)), k
    assert not np.array_equal(r["boxes"][0], r["boxes"][2])  # the moved copies have their own roots
    r = E.sky_record(MATS, cubes)
    assert (r["on"], r["n"], r["brute"]) == (0, 0, 0) and not r["boxes"].any()
    assert r["face"] == 0xFFFFFFFF and bits(r["t"])[0] == 0x7F7FFFFF  # the pixel is recorded all the same


def test_a_sphere_or_a_plane_switches_it_off():
    p = part("Cube")
    for ns, npl in ((1, 0), (0, 1), (2, 3)):
        r = E.sky_record(MATS, [p], ns, npl)
        assert (r["on"], r["n"]) == (0, 0) and not r["boxes"].any(), (ns, npl)
    assert E.sky_record(MATS, [p], 0, 0)["on"] == 1


def test_a_scene_without_models_is_all_sky():
    r = E.sky_record(MATS, [])
    assert (r["on"], r["n"], r["brute"]) == (1, 0, 0) and not r["boxes"].any()
