// The lock-free, order-independent union-find that pn_cluster.hip (voxel connected components) and pn_dbscan.hip (density clusters)
// share: one definition, two users.  parent[x] <= x always and a hook only ever gives a ROOT a smaller parent, so there are no
// cycles, ancestors stay ancestors, and the root of a finished tree is the set's lowest member whatever the interleaving.  Every
// access of parent[] here is a relaxed agent-scope atomic (the XCDs' L2s are not coherent; the word is its own payload), and no
// caller waits for another.  Bounds: a path has at most n nodes (parent strictly decreases), and a compare-and-swap fails only because
// another hook succeeded on that root, of which there are at most n - 1: with bound = n + 1 every find and every retry loop ends, and
// a loop that used its bound up reports VX_ERR_UNION.
#pragma once
#include "pn_voxel_grid.h"

namespace pn {

__device__ __forceinline__ int cl_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x in the forest as it is being built; *ok = false when the bound ran out
__device__ __forceinline__ int cl_find(const int* parent, int x, int bound, bool* ok) {
  int it = 0;
  for (;;) {
    const int p = cl_ld(parent + x);
    if (p == x) return x;
    if (p < 0 || p > x || ++it > bound) { *ok = false; return x; }
    x = p;
  }
}

// joins the trees of a and b; returns the root they share afterwards as this lane saw it (a lower bound for later walks from a)
__device__ __forceinline__ int cl_unite(int* parent, int a, int b, int bound, int* err) {
  bool ok = true;
  const int b0 = b;
  for (int it = 0; it <= bound; ++it) {
    const int ra = cl_find(parent, a, bound, &ok), rb = cl_find(parent, b, bound, &ok);
    if (!ok) break;
    if (ra == rb) {
      // shorten the next walk from b: ra is an ancestor of it, and a non-root's parent is only ever lowered to an ancestor
      if (ra < b0) __hip_atomic_fetch_min(parent + b0, ra, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return ra;
    }
    const int hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    int expected = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return lo;
    a = hi; b = lo;                        // hi got a parent meanwhile: walk on from the two old roots
  }
  atomicCAS(err, 0, (int)VX_ERR_UNION);
  return a;
}

}  // namespace pn
