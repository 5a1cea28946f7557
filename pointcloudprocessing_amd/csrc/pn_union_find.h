// What the two component labellers share (pn_cluster.hip: voxel connected components; pn_dbscan.hip: density clusters): the
// lock-free, order-independent union-find and the tail that turns its finished forest into dense ids -- one definition of each.
//
// Union-find.  parent[x] <= x always and a hook only ever gives a ROOT a smaller parent, so there are no cycles, ancestors stay
// ancestors, and the root of a finished tree is the set's lowest member whatever the interleaving.  Every access of parent[] by
// cl_find / cl_unite is a relaxed agent-scope atomic (the XCDs' L2s are not coherent; the word is its own payload), and no caller
// waits for another.  Bounds: a path has at most n nodes (parent strictly decreases), and a compare-and-swap fails only because
// another hook succeeded on that root, of which there are at most n - 1: with bound = n + 1 every find and every retry loop ends,
// and a loop that used its bound up reports VX_ERR_UNION.
//
// Tail.  settle the roots (cl_settled_root) -> flag what gets an id -> count the flags per block (cl_block_count) -> one workgroup
// scans the counts (cl_scan_kernel) -> a flag's rank is its id (cl_flag_rank) -> per-id sums and minima, a wave serving its commonest
// ids once each (cl_wave_grouped).  What is flagged (a root voxel; a row that is some root's lowest) is the caller's.  The block
// helpers are for workgroups of CL_T = 256 threads, four waves, and take four ints of LDS.
#pragma once
#include "pn_voxel_grid.h"

namespace pn {

constexpr int CL_T = 256;
static_assert(CL_T == 4 * 64, "cl_block_count, cl_flag_rank and vx_block_scan256 add four wave counts");

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

// root of x in the FINISHED forest; *ok = false when the walk is not one.  Plain loads: it runs in a launch of its own after the
// hooks' launch, which is why it is not cl_find
__device__ __forceinline__ int cl_settled_root(const int* __restrict__ parent, int x, int bound, bool* ok) {
  int it = 0;
  for (;;) {
    const int p = parent[x];
    if (p == x) return x;
    if (p < 0 || p > x || ++it > bound) { *ok = false; return x; }
    x = p;
  }
}

// bsum[blockIdx.x] = the workgroup's number of set flags (every thread calls it)
__device__ __forceinline__ void cl_block_count(bool flag, int* wcnt, int* __restrict__ bsum) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// the rank of this thread's set flag among all flags in thread order, -1 without one (every thread calls it); bofs: cl_scan_kernel's
__device__ __forceinline__ int cl_flag_rank(bool flag, const int* __restrict__ bofs, int* wcnt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) wcnt[wave] = __popcll(m);
  __syncthreads();
  if (!flag) return -1;
  int c = bofs[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) c += wcnt[w];
  return c;
}

// one workgroup: bofs = exclusive scan of bsum[0, nb), n_out[1] = the number of flags; n_out[0] = *n0 where the caller has one
// (static: the one definition is compiled into either file's code object)
static __global__ __launch_bounds__(CL_T) void cl_scan_kernel(const int* __restrict__ bsum, int nb, const int* __restrict__ n0,
                                                              int* __restrict__ bofs, int* __restrict__ n_out) {
  __shared__ int wsum[CL_T / 64];
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += CL_T) {
    const int i = b0 + threadIdx.x;
    const int c = i < nb ? bsum[i] : 0;
    int total;
    const int s = vx_block_scan256(c, wsum, &total);
    if (i < nb) bofs[i] = carry + s - c;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (n0) n_out[0] = *n0;
    n_out[1] = carry;
  }
}

// Every lane of a wave hands in a key (< 0: none; else an address the caller has range-checked) and a value.  Neighbouring lanes
// mostly share a key, and one large body would send every lane's atomic to one address: so the wave serves its first four distinct
// keys group by group -- the group's values folded across the wave (fold(a, b), `none` for the other lanes), commit(key, folded) once
// from the group's lowest lane -- and what is left lane by lane.  For integer sums and minima the grouping changes no result.
template <class Fold, class Commit>
__device__ __forceinline__ void cl_wave_grouped(int key, int val, int none, Fold&& fold, Commit&& commit) {
  for (int round = 0; round < 4; ++round) {
    const unsigned long long active = __ballot(key >= 0);
    if (active == 0ull) break;
    const int k0 = __shfl(key, __ffsll((long long)active) - 1, 64);
    const bool mine = key == k0;
    int v = mine ? val : none;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fold(v, __shfl_xor(v, o, 64));
    const unsigned long long group = __ballot(mine);
    if (mine) {
      if ((group & ((1ull << (threadIdx.x & 63)) - 1ull)) == 0ull) commit(k0, v);
      key = -1;
    }
  }
  if (key >= 0) commit(key, val);
}

}  // namespace pn
