// refs_budget.h -- the bound both octree builders (host_scene.cpp octree_build, build.hip
// build_levels) put on a tree's live primitive references: the primitives of every node that is a
// leaf so far or still waits to be split. The reference's vertex-in-box assignment (closed boxes)
// copies a triangle into every child it touches, so coincident triangles whose split point lies on
// a shared child-box face multiply per level until depth 64; a build whose references pass the
// budget returns ATR_E_NOMEM instead of asking for that memory. A split never lowers the sum (some
// vertex of every primitive lies in the node's box, hence in a child's), so the depth-first and
// the level-order builder refuse the same meshes. DESIGN.md (tree build) has the measured ratios.
// Plain C++ with no other include, so that a test can compile it alone.
#ifndef ATR_REFS_BUDGET_H
#define ATR_REFS_BUDGET_H
#include <cstdint>

namespace atr {

constexpr uint64_t kRefsBudgetCap = 0x7FFFFFFFull;  // 2^31 - 1
constexpr uint64_t kRefsBudgetPerFace = 256, kRefsBudgetFloor = 1ull << 20;

// min(2^31 - 1, 256 nfaces + 2^20), without overflow for any nfaces
constexpr uint64_t refs_budget(uint64_t nfaces) {
    return nfaces >= (kRefsBudgetCap - kRefsBudgetFloor) / kRefsBudgetPerFace + 1
               ? kRefsBudgetCap
               : kRefsBudgetPerFace * nfaces + kRefsBudgetFloor;
}

}  // namespace atr
#endif
