// The host builder of the per-part bounding-volume hierarchy that pn_icp_bvh_correspond / pn_semantic_icp_bvh search (pn_icp.hip:
// IcpBvh).  Host code only, no HIP call: a C user gets the tree Python gets.  The specification (split, numbering, boxes, padding)
// is in pointnet_hip.h, pn_icp_bvh_build; tests/icp_bvh_oracle.py checks the invariants and traverses the nodes in NumPy.
#include <algorithm>
#include <cmath>
#include <vector>

#include "pn_icp.h"

namespace pn {
namespace {

struct BvhBuild {
  const float* tri;
  pn_icp_bvh_node* nodes;
  int* rows;
  int n_nodes;
  std::vector<double> key;   // (T, 3): three times the centroid

  static float round_down(double v) {
    float f = (float)v;
    return (double)f > v ? std::nextafterf(f, -INFINITY) : f;
  }
  static float round_up(double v) {
    float f = (float)v;
    return (double)f < v ? std::nextafterf(f, INFINITY) : f;
  }

  // the exact box of rows[b .. e), moved outward by PN_ICP_BVH_PAD_ULPS ulp of the largest |coordinate|
  void leaf_box(int b, int e, pn_icp_bvh_node& n) const {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, m = 0.f;
    for (int i = b; i < e; ++i) {
      const float* t = tri + 9 * (long long)rows[i];
      for (int v = 0; v < 9; ++v) {
        lo[v % 3] = std::min(lo[v % 3], t[v]);
        hi[v % 3] = std::max(hi[v % 3], t[v]);
        m = std::max(m, std::fabs(t[v]));
      }
    }
    double pad = 0.0;
    if (m > 0.f) {
      int ex;
      std::frexp(m, &ex);                 // m = f * 2^ex, f in [0.5, 1): floor(log2 m) = ex - 1
      pad = PN_ICP_BVH_PAD_ULPS * std::ldexp(1.0, std::max(ex - 24, -149));
    }
    for (int k = 0; k < 3; ++k) {
      n.lo[k] = round_down((double)lo[k] - pad);
      n.hi[k] = round_up((double)hi[k] + pad);
    }
  }

  void node(int self, int b, int e) {
    pn_icp_bvh_node& n = nodes[self];
    if (e - b <= PN_ICP_BVH_LEAF) {
      leaf_box(b, e, n);
      n.first = b;
      n.count = e - b;
      return;
    }
    double kmin[3] = {INFINITY, INFINITY, INFINITY}, kmax[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = b; i < e; ++i)
      for (int k = 0; k < 3; ++k) {
        const double v = key[3 * (size_t)rows[i] + k];
        kmin[k] = std::min(kmin[k], v);
        kmax[k] = std::max(kmax[k], v);
      }
    int ax = 0;
    for (int k = 1; k < 3; ++k) ax = kmax[k] - kmin[k] > kmax[ax] - kmin[ax] ? k : ax;
    std::sort(rows + b, rows + e, [&](int x, int y) {
      const double kx = key[3 * (size_t)x + ax], ky = key[3 * (size_t)y + ax];
      return kx < ky || (kx == ky && x < y);
    });
    const int mid = b + (e - b) / 2, c0 = n_nodes;
    n_nodes += 2;
    node(c0, b, mid);
    node(c0 + 1, mid, e);
    const pn_icp_bvh_node &l = nodes[c0], &r = nodes[c0 + 1];
    for (int k = 0; k < 3; ++k) {
      nodes[self].lo[k] = std::min(l.lo[k], r.lo[k]);
      nodes[self].hi[k] = std::max(l.hi[k], r.hi[k]);
    }
    nodes[self].first = c0;
    nodes[self].count = 0;
  }
};

}  // namespace

// a label of T_l triangles has at most 2 T_l - 1 nodes
extern "C" int pn_icp_bvh_max_nodes(int T, int n_parts) { return T < 1 || T > (1 << 26) || n_parts < 1 ? 0 : 2 * T; }

extern "C" int pn_icp_bvh_build(const float* tri, const int32_t* tri_seg, int T, int n_parts, pn_icp_bvh_node* nodes, int32_t* rows,
                                int32_t* roots, int32_t* n_nodes) {
  const char* fn = "pn_icp_bvh_build";
  PN_CHECK_ARG(tri && tri_seg && nodes && rows && roots && n_nodes, "%s: null pointer (every argument is required)", fn);
  PN_CHECK_ARG(T >= 1 && T <= (1 << 26), "%s: T=%d outside [1, 2^26]", fn, T);
  PN_TRY(icp_check_seg(fn, tri_seg, T, n_parts));
  for (long long i = 0; i < 9ll * T; ++i)
    PN_CHECK_ARG(std::isfinite(tri[i]), "%s: vertex %lld of triangle %lld is not finite", fn, i % 9 / 3, i / 9);
  BvhBuild bb{tri, nodes, rows, 0, std::vector<double>(3 * (size_t)T)};
  for (int t = 0; t < T; ++t) {
    const float* v = tri + 9 * (long long)t;
    for (int k = 0; k < 3; ++k) bb.key[3 * (size_t)t + k] = ((double)v[k] + (double)v[3 + k]) + (double)v[6 + k];
    rows[t] = t;
  }
  for (int l = 0; l < n_parts; ++l) {
    roots[l] = -1;
    if (tri_seg[l + 1] == tri_seg[l]) continue;
    roots[l] = bb.n_nodes++;
    bb.node(roots[l], tri_seg[l], tri_seg[l + 1]);
  }
  *n_nodes = bb.n_nodes;
  return PN_OK;
}

}  // namespace pn
