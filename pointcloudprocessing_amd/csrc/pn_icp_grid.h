// The grid tables of a grouped reference cloud (pointnet_hip.h, pn_icp_grid_build): what pn_icp_grid.hip writes and the IcpGrid
// policy of pn_icp.hip's correspondence kernel reads.  One self-contained buffer in caller memory, laid out from its base and M
// alone, so the kernel argument is one pointer (IcpTree::grid, with IcpTree::T = M).
#pragma once
#include "pn_icp.h"
#include "pn_neighbors.h"

namespace pn {

// the head of the tables: what they were built for.  n_vox is written by the sort's heads kernel, the rest by the gather.
struct IcpGridHead {
  int n_vox;              // occupied voxels V
  int M;
  float r2, h;            // the largest max_d2 a search may pass, and the leaf derived from it (pn_icp_grid_leaf)
  float ox, oy, oz;       // the origin
  int pad;
};

struct IcpGridTab {
  const IcpGridHead* head;
  const float4* rec;                   // (M) x, y, z, grouped row as int bits, in grid order
  const unsigned long long* vkey;      // (M) the V occupied voxels' keys, ascending; ~0 behind them
  const int* vstart;                   // (M + 1) the voxels' first positions; M from V on
  size_t total;
};

__host__ __device__ __forceinline__ IcpGridTab icp_grid_carve(const void* base, int M) {
  const char* b = static_cast<const char*>(base);
  constexpr auto al = [](size_t v) constexpr { return (v + 255) & ~(size_t)255; };
  IcpGridTab g;
  size_t o = 0;
  g.head = reinterpret_cast<const IcpGridHead*>(b + o); o += al(sizeof(IcpGridHead));
  g.rec = reinterpret_cast<const float4*>(b + o); o += al((size_t)M * sizeof(float4));
  g.vkey = reinterpret_cast<const unsigned long long*>(b + o); o += al((size_t)M * sizeof(unsigned long long));
  g.vstart = reinterpret_cast<const int*>(b + o); o += al(((size_t)M + 1) * sizeof(int));
  g.total = o;
  return g;
}

}  // namespace pn
