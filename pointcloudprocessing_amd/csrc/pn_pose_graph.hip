// Pose-graph optimisation (gfx950): Levenberg-Marquardt over the K node poses of a multiway registration, given E pairwise edges
// with their information matrices.  The specification is build-defined and stated in pointnet_hip.h (pn_pose_graph_optimize), with
// the NumPy oracle in tests/pose_graph_oracle.py.
//
// One launch of ONE workgroup of 256 threads runs the whole solve in fp64: the problem is small (at most 378 unknowns, 4096 edges),
// strictly sequential across iterations and runs once per call, so what it costs is barriers, not arithmetic; a second workgroup
// would need a grid-wide meeting per phase.  No host read, every loop bounded by an argument or a constant, no spin wait:
// capturable.  Per iteration:
//   (once)         the weights as they count and the live edges (weight > 0) compacted in order: all below runs over these alone
//   pg_linearize   edges in parallel (one per thread, strided): r, J = [J_i | J_j] (6 x 12) into the workspace
//   pg_weigh       (edge, entry) pairs in parallel: WJ = w Lambda J (6 x 12) and Wr = w Lambda r
//   pg_assemble    H and g zeroed, then 36 threads add the four 6 x 6 blocks of J^T WJ of every live edge into H in edge order and 6
//                  more add J^T Wr into g: thread (r, c) owns entry (r, c) of every 6 x 6 block of H, so an address has one writer
//                  whichever edges meet at its node, and no atomic is needed
//   up to 10 tries pg_factor: H + lambda diag H -> L D L^T column by column, one barrier per column; pg_solve: the two triangular
//                  solves, one barrier per column; the trial poses X D(delta); pg_cost: the cost over the edges, a fixed tree
// H (at most 378^2 fp64 = 1.1 MB) and its factor live in the workspace and stay in L2; the factor is stored by columns
// (F[c * n + i] = entry (i, c)), so that the lanes of a column step, one row each, read consecutive addresses.  LDS holds only the
// solve's vector, the reciprocal pivots and the reduction tree (8 KB): one path for every graph size.
#include "pn_common.h"

namespace pn {

constexpr int PG_THREADS = 256;
constexpr int PG_MAX_N = 6 * (PN_POSE_GRAPH_MAX_NODES - 1);
constexpr int PG_TRIES = 10;

struct M3 {
  double m[9];
};
struct V3 {
  double x, y, z;
};

__device__ __forceinline__ M3 m3_mul(const M3& a, const M3& b) {   // a b
  M3 c;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) c.m[3 * r + k] = (a.m[3 * r] * b.m[k] + a.m[3 * r + 1] * b.m[3 + k]) + a.m[3 * r + 2] * b.m[6 + k];
  return c;
}
__device__ __forceinline__ M3 m3_tmul(const M3& a, const M3& b) {   // a^T b
  M3 c;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) c.m[3 * r + k] = (a.m[r] * b.m[k] + a.m[3 + r] * b.m[3 + k]) + a.m[6 + r] * b.m[6 + k];
  return c;
}
__device__ __forceinline__ M3 m3_t(const M3& a) {
  return M3{{a.m[0], a.m[3], a.m[6], a.m[1], a.m[4], a.m[7], a.m[2], a.m[5], a.m[8]}};
}
__device__ __forceinline__ V3 m3_vec(const M3& a, const V3& v) {
  return V3{(a.m[0] * v.x + a.m[1] * v.y) + a.m[2] * v.z, (a.m[3] * v.x + a.m[4] * v.y) + a.m[5] * v.z,
            (a.m[6] * v.x + a.m[7] * v.y) + a.m[8] * v.z};
}
__device__ __forceinline__ V3 m3_tvec(const M3& a, const V3& v) {
  return V3{(a.m[0] * v.x + a.m[3] * v.y) + a.m[6] * v.z, (a.m[1] * v.x + a.m[4] * v.y) + a.m[7] * v.z,
            (a.m[2] * v.x + a.m[5] * v.y) + a.m[8] * v.z};
}
__device__ __forceinline__ M3 m3_hat(const V3& v) { return M3{{0.0, -v.z, v.y, v.z, 0.0, -v.x, -v.y, v.x, 0.0}}; }

// [R t] of a row-major (4, 4) pose
__device__ __forceinline__ void pg_load(const double* P, M3& R, V3& t) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) R.m[3 * r + c] = P[4 * r + c];
  t = V3{P[3], P[7], P[11]};
}

// I + a K + b K^2, K = [w]_x, K^2 = w w^T - |w|^2 I
__device__ __forceinline__ M3 pg_series(const V3& w, double a, double b) {
  const double th2 = (w.x * w.x + w.y * w.y) + w.z * w.z;
  const double v[3] = {w.x, w.y, w.z};
  const M3 K = m3_hat(w);
  M3 o;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o.m[3 * r + c] = ((r == c ? 1.0 : 0.0) + a * K.m[3 * r + c]) + b * (v[r] * v[c] - (r == c ? th2 : 0.0));
  return o;
}

// what an edge's error is made of: E = Z^-1 X_i^-1 X_j = [RE tE], its rotation vector om and angle th, and X_i^-1 X_j = [Rij tij]
struct PgEdge {
  M3 RE, Rij;
  V3 tE, tij, om;
  double th;
};

__device__ __forceinline__ PgEdge pg_edge(const double* Xi, const double* Xj, const double* Zk) {
  M3 Ri, Rj, Rz;
  V3 ti, tj, tz;
  pg_load(Xi, Ri, ti);
  pg_load(Xj, Rj, tj);
  pg_load(Zk, Rz, tz);
  PgEdge e;
  e.Rij = m3_tmul(Ri, Rj);
  e.tij = m3_tvec(Ri, V3{tj.x - ti.x, tj.y - ti.y, tj.z - ti.z});
  e.RE = m3_tmul(Rz, e.Rij);
  e.tE = m3_tvec(Rz, V3{e.tij.x - tz.x, e.tij.y - tz.y, e.tij.z - tz.z});
  const M3& R = e.RE;
  const V3 s{0.5 * (R.m[7] - R.m[5]), 0.5 * (R.m[2] - R.m[6]), 0.5 * (R.m[3] - R.m[1])};
  const double c = 0.5 * (((R.m[0] + R.m[4]) + R.m[8]) - 1.0);
  const double sn = sqrt((s.x * s.x + s.y * s.y) + s.z * s.z);
  e.th = atan2(sn, c);
  const double f = sn < 1e-12 ? 1.0 : e.th / sn;
  e.om = V3{s.x * f, s.y * f, s.z * f};
  return e;
}

// w r^T Lambda r of one edge
__device__ __forceinline__ double pg_edge_cost(const PgEdge& e, const double* __restrict__ L, double w) {
  const double r[6] = {e.om.x, e.om.y, e.om.z, e.tE.x, e.tE.y, e.tE.z};
  double acc = 0.0;
#pragma unroll
  for (int p = 0; p < 6; ++p) {
    double lr = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) lr += L[6 * p + q] * r[q];
    acc += r[p] * lr;
  }
  return w * acc;
}

// the workspace, in doubles
struct PgWs {
  double *J, *WJ, *r, *Wr, *w, *H, *F, *g, *Xt;
  int* live;               // the live edges (weight > 0), ascending
  size_t doubles;
};

static inline PgWs pg_layout(void* ws, int K, int E) {
  const size_t n = 6 * (size_t)(K - 1), e = (size_t)E;
  double* base = static_cast<double*>(ws);
  size_t o = 0;
  PgWs w;
  w.J = base + o; o += e * 72;
  w.WJ = base + o; o += e * 72;
  w.r = base + o; o += e * 6;
  w.Wr = base + o; o += e * 6;
  w.w = base + o; o += e;
  w.H = base + o; o += n * n;
  w.F = base + o; o += n * n;
  w.g = base + o; o += n;
  w.Xt = base + o; o += (size_t)K * 16;
  w.live = reinterpret_cast<int*>(base + o); o += (e + 1) / 2;
  w.doubles = o;
  return w;
}

// the cost at the poses X over the L live edges: per thread over the live edges number t, t + 256, .. ascending, then a fixed
// tree.  Every thread calls it and gets the same value.
__device__ double pg_cost(const double* X, int L, const int* live, const int* __restrict__ edges, const double* __restrict__ Z,
                          const double* __restrict__ info, const double* wk, double* s_red) {
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int m = tid; m < L; m += PG_THREADS) {
    const int k = live[m];
    const PgEdge e = pg_edge(X + 16 * edges[2 * k], X + 16 * edges[2 * k + 1], Z + 16 * (size_t)k);
    acc += pg_edge_cost(e, info + 36 * (size_t)k, wk[k]);
  }
  __syncthreads();                       // (s_red may still be read from the call before)
  s_red[tid] = acc;
  __syncthreads();
  for (int h = PG_THREADS / 2; h > 0; h >>= 1) {
    if (tid < h) s_red[tid] = s_red[tid] + s_red[tid + h];
    __syncthreads();
  }
  return s_red[0];
}

// r and J = [J_i | J_j] of every live edge at the poses X
__device__ void pg_linearize(const double* X, int L, const int* live, const int* __restrict__ edges, const double* __restrict__ Z,
                             double* __restrict__ Jo, double* __restrict__ ro) {
  for (int m = threadIdx.x; m < L; m += PG_THREADS) {
    const int k = live[m];
    const PgEdge e = pg_edge(X + 16 * edges[2 * k], X + 16 * edges[2 * k + 1], Z + 16 * (size_t)k);
    const double th = e.th;
    const double b = th < 1e-4 ? 1.0 / 12.0 : 1.0 / (th * th) - (1.0 + cos(th)) / ((2.0 * th) * sin(th));
    const M3 A = pg_series(e.om, 0.5, b);                       // Jr^-1(omega)
    // T = X_j^-1 X_i = [RT tT]; J_i = -[[A RT, 0], [RE [tT]_x RT, RE RT]]
    const M3 RT = m3_t(e.Rij);
    const V3 u = m3_tvec(e.Rij, e.tij);
    const V3 tT{-u.x, -u.y, -u.z};
    const M3 Bm = m3_mul(A, RT);
    const M3 Dm = m3_mul(e.RE, RT);
    const M3 Cm = m3_mul(e.RE, m3_mul(m3_hat(tT), RT));
    double* J = Jo + 72 * (size_t)m;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        J[12 * p + c] = -Bm.m[3 * p + c];
        J[12 * p + 3 + c] = 0.0;
        J[12 * p + 6 + c] = A.m[3 * p + c];
        J[12 * p + 9 + c] = 0.0;
        J[12 * (p + 3) + c] = -Cm.m[3 * p + c];
        J[12 * (p + 3) + 3 + c] = -Dm.m[3 * p + c];
        J[12 * (p + 3) + 6 + c] = 0.0;
        J[12 * (p + 3) + 9 + c] = e.RE.m[3 * p + c];
      }
    }
    double* r = ro + 6 * (size_t)m;
    r[0] = e.om.x; r[1] = e.om.y; r[2] = e.om.z;
    r[3] = e.tE.x; r[4] = e.tE.y; r[5] = e.tE.z;
  }
}

__global__ __launch_bounds__(PG_THREADS) void pose_graph_kernel(int K, int E, const int* __restrict__ edges, const double* __restrict__ Z,
                                                                const double* __restrict__ info, const double* __restrict__ edge_weight,
                                                                double* X, int max_iters, double tol, double lambda0, PgWs ws,
                                                                double* __restrict__ cost_out, int* __restrict__ iters_out,
                                                                int* __restrict__ status_out) {
  __shared__ double s_red[PG_THREADS];
  __shared__ double s_y[PG_MAX_N];
  __shared__ double s_ip[PG_MAX_N];      // 1 / d_c
  __shared__ int s_cnt[PG_THREADS];
  __shared__ int s_live;
  const int tid = threadIdx.x;
  const int n = 6 * (K - 1);

  // the edge list, before anything is written
  int bad = 0;
  for (int k = tid; k < E; k += PG_THREADS) {
    const int i = edges[2 * k], j = edges[2 * k + 1];
    bad |= (unsigned)i >= (unsigned)K || (unsigned)j >= (unsigned)K || i == j;
  }
  if (__syncthreads_or(bad)) {
    if (tid == 0) {
      cost_out[0] = __builtin_nan("");
      cost_out[1] = __builtin_nan("");
      iters_out[0] = 0;
      status_out[0] = PN_POSE_GRAPH_BAD_EDGE;
    }
    return;
  }
  // the weights as they count, and the live edges compacted in ascending order (a chunk of edges per thread, the chunks' counts
  // scanned by thread 0): everything below runs over the live edges alone, so an edge of weight 0 is an edge that is not there
  const int chunk = (E + PG_THREADS - 1) / PG_THREADS, k0 = min(tid * chunk, E), k1 = min(k0 + chunk, E);
  int cnt = 0;
  for (int k = k0; k < k1; ++k) {
    const double w = edge_weight ? edge_weight[k] : 1.0;
    const bool on = w > 0.0 && __builtin_isfinite(w);
    ws.w[k] = on ? w : 0.0;
    cnt += on ? 1 : 0;
  }
  s_cnt[tid] = cnt;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int t = 0; t < PG_THREADS; ++t) { const int c = s_cnt[t]; s_cnt[t] = run; run += c; }
    s_live = run;
  }
  __syncthreads();
  {
    int at = s_cnt[tid];
    for (int k = k0; k < k1; ++k)
      if (ws.w[k] > 0.0) ws.live[at++] = k;
  }
  __syncthreads();
  const int L = s_live;

  double cost = pg_cost(X, L, ws.live, edges, Z, info, ws.w, s_red);
  const double cost0 = cost;
  double lambda = lambda0;
  int status = PN_POSE_GRAPH_MAX_ITERS, it = 0;
  for (; it < max_iters;) {
    ++it;
    pg_linearize(X, L, ws.live, edges, Z, ws.J, ws.r);
    for (int e = tid; e < n * n; e += PG_THREADS) ws.H[e] = 0.0;
    for (int e = tid; e < n; e += PG_THREADS) ws.g[e] = 0.0;
    __syncthreads();
    // WJ = w Lambda J (6 x 12) and Wr = w Lambda r (6) of every live edge, one entry per thread and round
    for (int e = tid; e < L * 78; e += PG_THREADS) {
      const int m = e / 78, s = e % 78, k = ws.live[m];
      const double w = ws.w[k];
      const double* La = info + 36 * (size_t)k;
      if (s < 72) {
        const int p = s / 12, c = s % 12;
        const double* J = ws.J + 72 * (size_t)m;
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) a += La[6 * p + q] * J[12 * q + c];
        ws.WJ[72 * (size_t)m + s] = w * a;
      } else {
        const int p = s - 72;
        const double* r = ws.r + 6 * (size_t)m;
        double a = 0.0;
#pragma unroll
        for (int q = 0; q < 6; ++q) a += La[6 * p + q] * r[q];
        ws.Wr[6 * (size_t)m + p] = w * a;
      }
    }
    __syncthreads();
    // H and g in edge order.  Thread t < 36 owns entry (t / 6, t % 6) of EVERY 6 x 6 block of H, whichever nodes the block belongs to,
    // and adds the four blocks of an edge itself; threads 36 .. 41 own an entry of every node's part of g.  An address of H or g is
    // thus written by one thread only, edge after edge: two edges that share a node do not race (a node is i in one edge and j in
    // another, so ownership by the position in the edge's 12 x 12 block would), and no atomic is needed.
    if (tid < 42) {
      const bool isg = tid >= 36;
      const int r6 = isg ? tid - 36 : tid / 6, c6 = isg ? 0 : tid % 6;
      for (int m = 0; m < L; ++m) {
        const int k = ws.live[m];
        const int node[2] = {edges[2 * k], edges[2 * k + 1]};
        const double* J = ws.J + 72 * (size_t)m;
        const double* WJ = ws.WJ + 72 * (size_t)m;
        const double* Wr = ws.Wr + 6 * (size_t)m;
#pragma unroll
        for (int ha = 0; ha < 2; ++ha) {
          const int a = node[ha];
          if (a == 0) continue;
          const int row = 6 * (a - 1) + r6;
          if (isg) {
            double v = 0.0;
#pragma unroll
            for (int p = 0; p < 6; ++p) v += J[12 * p + 6 * ha + r6] * Wr[p];
            ws.g[row] = ws.g[row] + v;
            continue;
          }
#pragma unroll
          for (int hb = 0; hb < 2; ++hb) {
            const int b = node[hb];
            if (b == 0) continue;
            double v = 0.0;
#pragma unroll
            for (int p = 0; p < 6; ++p) v += J[12 * p + 6 * ha + r6] * WJ[12 * p + 6 * hb + c6];
            double* h = ws.H + (size_t)row * n + 6 * (b - 1) + c6;
            *h = *h + v;
          }
        }
      }
    }
    __syncthreads();

    bool accepted = false, singular = false;
    double dmax = 0.0;
    for (int tr = 0; tr < PG_TRIES && !accepted; ++tr) {
      // F <- H + lambda diag H (symmetric: column c holds row c)
      for (int e = tid; e < n * n; e += PG_THREADS) {
        const int c = e / n, i = e % n;
        const double h = ws.H[e];
        ws.F[e] = c == i ? h + lambda * h : h;
      }
      __syncthreads();
      // L D L^T, left-looking: after step c, F[c * n + i] = u_ic = L_ic d_c for i > c and F[c * n + c] = d_c
      for (int c = 0; c < n; ++c) {
        for (int i = c + tid; i < n; i += PG_THREADS) {
          double s = ws.F[(size_t)c * n + i];
          for (int k = 0; k < c; ++k) s -= ws.F[(size_t)k * n + i] * (ws.F[(size_t)k * n + c] * s_ip[k]);
          ws.F[(size_t)c * n + i] = s;
          if (i == c) s_ip[c] = 1.0 / s;
        }
        __syncthreads();
        const double d = ws.F[(size_t)c * n + c];
        if (!(d > 0.0 && __builtin_isfinite(d))) { singular = true; break; }
      }
      if (singular) break;
      // L y = -g
      for (int i = tid; i < n; i += PG_THREADS) s_y[i] = -ws.g[i];
      __syncthreads();
      for (int c = 0; c < n - 1; ++c) {
        const double yc = s_y[c] * s_ip[c];
        for (int i = c + 1 + tid; i < n; i += PG_THREADS) s_y[i] -= ws.F[(size_t)c * n + i] * yc;
        __syncthreads();
      }
      // D z = y, then L^T delta = z by columns from the last
      for (int i = tid; i < n; i += PG_THREADS) s_y[i] = s_y[i] * s_ip[i];
      __syncthreads();
      for (int c = n - 1; c > 0; --c) {
        const double xc = s_y[c];
        for (int k = tid; k < c; k += PG_THREADS) s_y[k] -= (ws.F[(size_t)k * n + c] * s_ip[k]) * xc;
        __syncthreads();
      }
      // trial poses X D(delta); node 0 as it is
      for (int a = tid; a < K; a += PG_THREADS) {
        const double* P = X + 16 * a;
        double* Q = ws.Xt + 16 * a;
        if (a == 0) {
          for (int e = 0; e < 16; ++e) Q[e] = P[e];
          continue;
        }
        const double* dl = s_y + 6 * (a - 1);
        const V3 w{dl[0], dl[1], dl[2]}, v{dl[3], dl[4], dl[5]};
        const double th = sqrt((w.x * w.x + w.y * w.y) + w.z * w.z);
        double ca = 1.0, cb = 0.0;
        if (!(th < 1e-12)) {
          const double h = sin(0.5 * th) / th;
          ca = sin(th) / th;
          cb = 2.0 * h * h;
        }
        M3 R;
        V3 t;
        pg_load(P, R, t);
        const M3 Rn = m3_mul(R, pg_series(w, ca, cb));
        const V3 dv = m3_vec(R, v);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int c = 0; c < 3; ++c) Q[4 * r + c] = Rn.m[3 * r + c];
        Q[3] = t.x + dv.x; Q[7] = t.y + dv.y; Q[11] = t.z + dv.z;
        for (int e = 12; e < 16; ++e) Q[e] = P[e];
      }
      __syncthreads();
      const double trial = pg_cost(ws.Xt, L, ws.live, edges, Z, info, ws.w, s_red);
      if (trial <= cost) {
        accepted = true;
        cost = trial;
        lambda = fmax(lambda / 10.0, 1e-12);
        dmax = 0.0;
        for (int e = 0; e < n; ++e) dmax = fmax(dmax, fabs(s_y[e]));
        for (int e = 16 + tid; e < 16 * K; e += PG_THREADS) X[e] = ws.Xt[e];
      } else {
        lambda = 10.0 * lambda;
      }
      __syncthreads();                   // X is complete, and s_y is free again
    }
    if (singular) { status = PN_POSE_GRAPH_SINGULAR; break; }
    if (!accepted || dmax < tol) { status = 0; break; }
  }
  if (tid == 0) {
    cost_out[0] = cost0;
    cost_out[1] = cost;
    iters_out[0] = it;
    status_out[0] = status;
  }
}

}  // namespace pn

using namespace pn;

extern "C" {

size_t pn_pose_graph_workspace_bytes(int K, int E) {
  if (K < 2 || K > PN_POSE_GRAPH_MAX_NODES || E < K - 1 || E > PN_POSE_GRAPH_MAX_EDGES) return 0;
  return pg_layout(nullptr, K, E).doubles * sizeof(double);
}

int pn_pose_graph_optimize(int K, int E, const int32_t* edges, const double* Z, const double* info, const double* edge_weight,
                           double* poses_inout, int max_iters, double tol, double lambda0, double* cost_out, int32_t* iters_out,
                           int32_t* status_out, void* workspace, size_t workspace_bytes, pn_stream stream) {
  const char* fn = "pn_pose_graph_optimize";
  PN_CHECK_ARG(edges && Z && info && poses_inout && cost_out && iters_out && status_out && workspace,
               "%s: null pointer (everything but edge_weight is required)", fn);
  PN_CHECK_ARG(K >= 2 && K <= PN_POSE_GRAPH_MAX_NODES, "%s: K=%d outside [2, %d]", fn, K, PN_POSE_GRAPH_MAX_NODES);
  PN_CHECK_ARG(E >= K - 1 && E <= PN_POSE_GRAPH_MAX_EDGES, "%s: E=%d outside [K - 1 = %d, %d]", fn, E, K - 1, PN_POSE_GRAPH_MAX_EDGES);
  PN_CHECK_ARG(max_iters >= 1 && max_iters <= 10000, "%s: max_iters=%d outside [1, 10000]", fn, max_iters);
  PN_CHECK_ARG(tol >= 0.0, "%s: tol=%g must be >= 0", fn, tol);
  PN_CHECK_ARG(lambda0 > 0.0 && lambda0 <= 1.7976931348623157e308, "%s: lambda0=%g must be > 0 and finite", fn, lambda0);
  PN_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "%s: workspace must be 8-byte aligned", fn);
  const size_t need = pn_pose_graph_workspace_bytes(K, E);
  PN_CHECK_ARG(workspace_bytes >= need, "%s: workspace of %zu bytes, %zu required", fn, workspace_bytes, need);
  hipLaunchKernelGGL(pose_graph_kernel, dim3(1), dim3(PG_THREADS), 0, S(stream), K, E, edges, Z, info, edge_weight, poses_inout, max_iters,
                     tol, lambda0, pg_layout(workspace, K, E), cost_out, iters_out, status_out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // extern "C"
