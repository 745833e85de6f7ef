"""atr_octree_build on meshes whose reference build never ends (no GPU): coincident triangles in an
axis-aligned plane have their split point on a shared child-box face, the closed point-in-box test
hands all of them to two or more children, and the references double per level down to depth 64. The
builders bound a tree's live primitive references by refs_budget (atray_amd/csrc/refs_budget.h) and
return ATR_E_NOMEM; no exception crosses the C ABI. Every build here runs in a fresh child process
under an 8 GB address-space limit and a 60 s timeout, so that a regression fails a test instead of
taking pytest down. The oracle restates the reference and does not end on these inputs either: the
runaway meshes are never handed to it. The device builder's guard is the same function applied to
each level's counts before the next level is allocated; it is not provoked on a GPU."""
import json
import os
import resource
import subprocess
import sys

import pytest

from tests import scale_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 8 << 30
TRI = "v 0 0 0\nv 1 0 0\nv 0 1 0\n"
TILTED = "v 0 0 0\nv 1 0 0\nv 0 1 1\n"

CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
from atray_amd import engine as E
m = E.Mesh.parse_obj(open(sys.argv[2]).read())
try:
    st = E.Octree.build(m, int(sys.argv[3])).stats()
    print(json.dumps({"rc": "ATR_OK", "stats": st}))
except E.AtrError as e:
    print(json.dumps({"rc": str(e)}))
"""


def _limit():
    resource.setrlimit(resource.RLIMIT_AS, (LIMIT, LIMIT))


def build_in_child(tmp_path, text, leaf):
    """E.Octree.build of an OBJ text in a child process: its exit status and what it reported."""
    path = tmp_path / "mesh.obj"
    path.write_text(text)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path), str(leaf)], capture_output=True, text=True,
                       timeout=60, preexec_fn=_limit)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def monkey_at(c):
    return S.obj_text([("Monkey", S.place("Monkey", 1.0, c))])


RUNAWAY = {
    "two_coincident_leaf1": (lambda: TRI + "f 1 2 3\n" * 2, 1),
    "65_coincident_leaf64": (lambda: TRI + "f 1 2 3\n" * 65, 64),
    "monkey_at_2^23": (lambda: monkey_at((2.0 ** 23, 2.0 ** 23, 2.0 ** 23)), 64),
    "monkey_at_2^22": (lambda: monkey_at((2.0 ** 22, 2.0 ** 22, -2.0 ** 22)), 64),
}
# the same shapes just off the runaway condition: they build, deep, and equal the oracle's tree
NEAR = {
    "65_tilted_leaf64": (TILTED + "f 1 2 3\n" * 65, 64, 1521),
    "two_sharing_an_edge_leaf1": ("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 1\nf 1 2 3\nf 1 2 4\n", 1, 1017),
}


@pytest.mark.parametrize("name", list(RUNAWAY))
def test_runaway_build_returns_nomem(tmp_path, name):
    make, leaf = RUNAWAY[name]
    got = build_in_child(tmp_path, make(), leaf)
    assert "ATR_E_NOMEM" in got["rc"], got


@pytest.mark.parametrize("name", list(NEAR))
def test_near_misses_still_build_and_match_the_oracle(tmp_path, name):
    from atray_amd import engine as E
    from oracle import oracle as O
    from tests.test_capi_host import same_tree
    text, leaf, nodes = NEAR[name]
    got = build_in_child(tmp_path, text, leaf)  # first where a runaway would be contained
    assert got["rc"] == "ATR_OK" and got["stats"]["nodes"] == nodes, got
    s = O.Scene(obj_text=text, center=None, max_faces=leaf)
    t = E.Octree.build(E.Mesh.parse_obj(text), leaf)
    same_tree(t, s)
    assert t.stats()["nodes"] == s.tree_stats()["nodes"] == nodes


def test_refs_budget_values(tmp_path):
    """min(2^31 - 1, 256 nfaces + 2^20) at 0, 1, 2^23 and 2^31 faces, from the header itself."""
    src = tmp_path / "budget.cpp"
    src.write_text('#include <cstdio>\n#include "refs_budget.h"\nint main() {\n'
                   '    const unsigned long long n[4] = {0ull, 1ull, 1ull << 23, 1ull << 31};\n'
                   '    for (int i = 0; i < 4; ++i) std::printf("%llu\\n", (unsigned long long)atr::refs_budget(n[i]));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "budget"
    subprocess.run(["c++", "-std=c++17", "-I", os.path.join(ROOT, "atray_amd", "csrc"), "-o", str(exe), str(src)],
                   check=True, capture_output=True, timeout=60)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=10).stdout.split()
    assert [int(x) for x in out] == [2 ** 20, 2 ** 20 + 256, 2 ** 31 - 1, 2 ** 31 - 1]



BARRIER_CHILD = """
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
from atray_amd import engine as E
W = 1 << 20
arr, n = E.tiles_array([[0, 0, W - 1, W - 1]])
t = C.cast(arr, C.c_void_p)
L = E.lib()
print(json.dumps([int(L.atr_packed_pixel_map(t, n, W, W, None, 0)), int(L.atr_render_packed_size(t, n))]))
"""


def test_count_returning_entry_points_report_nomem():
    """A 2^20 x 2^20 tile needs 2^34 work blocks: atr_packed_pixel_map and atr_render_packed_size, which
    return counts, hand the std::bad_alloc back as the negative ATR_E_NOMEM instead of ending the caller."""
    r = subprocess.run([sys.executable, "-c", BARRIER_CHILD, ROOT], capture_output=True, text=True, timeout=60,
                       preexec_fn=_limit)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert json.loads(r.stdout.strip().splitlines()[-1]) == [-3, -3]
