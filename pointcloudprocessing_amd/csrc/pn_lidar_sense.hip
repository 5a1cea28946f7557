// The sensor model between pn_lidar_cast and pn_lidar_pack (gfx950): pn_lidar_sense turns the ideal first-hit returns of a cast
// into what a flash LiDAR reports -- returns lost to grazing incidence and to the detection threshold (received power ~ cos / range^2),
// mixed pixels on range discontinuities, and range noise that grows with range.  The specification is build-defined and stated in
// pointnet_hip.h (pn_lidar_sense), with the NumPy oracle in tests/lidar_sense_oracle.py: seeded, a pure function of the inputs,
// bit for bit the oracle's.
//
// One launch.  One ray per lane, a wave takes 64 consecutive rays of one frame (a piece of an image row, or the seam of two),
// blockIdx.y is the frame (frames beyond the grid's y limit follow in a stride).  Per ray: its own (hit, t), the nine floats of its
// triangle (a gather through hit, the only divergent load), the (hit, t) of its four image neighbours (rows i - W, i - 1, i + 1,
// i + W of the INPUT: a ray's fate never depends on another ray's draws, so nothing is exchanged), two Philox4x32-10 blocks, and
// a few dozen fp64 operations without contraction.  No LDS, no atomics, no workspace, no host read.  The cost does not depend on
// the mesh: B * H * W rays against the cast's B * H * W * T tests.
#include "pn_philox.h"

namespace pn {

constexpr int LS_THREADS = 256;                 // rays per block (4 waves)
constexpr int LS_MAX_GRID_Y = 65535;
constexpr unsigned LS_DOMAIN = 0x53454E53u;     // "SENS": the fourth counter word, apart from pn_mesh_sample's and pn_plane_segment's draws

struct LidarSensor {
  double sigma0, sigma1;        // range noise: metres, metres per metre
  double strength, range_ref;   // detection; strength = +inf: no test
  double min_cos2;              // incidence cut; 0: none
  double jump, p_mix;           // mixed pixels; p_mix = 0: none
};

// U(w) of the header: the top 24 bits of a word as a double in [0, 1)
__device__ __forceinline__ double lidar_u24(unsigned w) { return (double)(w >> 8) * 0x1p-24; }

// one image neighbour (row k of the frame) of a ray of range t: its range difference replaces the partner's when it is a return,
// exceeds the jump and is larger than the best so far (strictly: the first in the header's order wins a tie; a NaN never does)
__device__ __forceinline__ void lidar_partner(const int* __restrict__ hit, const float* __restrict__ t, long long k, int T, double tt,
                                              double jump, double& best, double& best_abs, bool& have) {
#pragma clang fp contract(off)
  const int hn = hit[k];
  if (hn < 0 || hn >= T) return;
  const double dj = (double)t[k] - tt, a = fabs(dj);
  const bool take = (a > jump) & (!have | (a > best_abs));
  best = take ? dj : best;
  best_abs = take ? a : best_abs;
  have |= take;
}

__global__ __launch_bounds__(LS_THREADS) void lidar_sense_kernel(const float* __restrict__ tri, int T, const float* __restrict__ poses, int B,
                                                                const float* __restrict__ dirs, int H, int W, const int* __restrict__ hit,
                                                                const float* __restrict__ t, unsigned key0, unsigned key1, int frame0,
                                                                LidarSensor m, int* __restrict__ hit_out, float* __restrict__ t_out,
                                                                unsigned char* __restrict__ kind_out) {
#pragma clang fp contract(off)
  const int R = H * W;
  const int i = blockIdx.x * LS_THREADS + threadIdx.x;
  if (i >= R) return;
  const int r = i / W, c = i - r * W;
  const float sdx = dirs[3 * i], sdy = dirs[3 * i + 1], sdz = dirs[3 * i + 2];
  const bool detect = __builtin_isfinite(m.strength);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const long long base = (long long)b * R, row = base + i;
    const int h = hit[row];
    int ho = -1;
    float to = INFINITY;
    unsigned char kind = PN_LIDAR_MISS;
    if (h >= 0 && h < T) {
      kind = PN_LIDAR_DROPPED;
      const double tt = (double)t[row];
      // incidence: the face normal and the ray in the model frame (the cast's fp32 R^T dir, widened)
      const float* P = poses + 16 * (long long)b;
      const double dx = (double)((P[0] * sdx + P[4] * sdy) + P[8] * sdz);
      const double dy = (double)((P[1] * sdx + P[5] * sdy) + P[9] * sdz);
      const double dz = (double)((P[2] * sdx + P[6] * sdy) + P[10] * sdz);
      const float* v = tri + 9 * (long long)h;
      const double ax = (double)v[0], ay = (double)v[1], az = (double)v[2];
      const double e1x = (double)v[3] - ax, e1y = (double)v[4] - ay, e1z = (double)v[5] - az;
      const double e2x = (double)v[6] - ax, e2y = (double)v[7] - ay, e2z = (double)v[8] - az;
      const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
      const double nd = (nx * dx + ny * dy) + nz * dz;
      const double nn = (nx * nx + ny * ny) + nz * nz;
      const double dd = (dx * dx + dy * dy) + dz * dz;
      const double q = nn * dd;
      const double cs = (__builtin_isfinite(q) && q > 0.0) ? fabs(nd) / __dsqrt_rn(q) : 1.0;
      unsigned x[4], y[4];
      philox4x32_10((unsigned)i, (unsigned)(frame0 + b), 0u, LS_DOMAIN, key0, key1, x);
      philox4x32_10((unsigned)i, (unsigned)(frame0 + b), 1u, LS_DOMAIN, key0, key1, y);
      bool drop = cs * cs < m.min_cos2;
      if (detect) {
        const double rr = m.range_ref / tt;
        const double p = ((m.strength * cs) * rr) * rr;
        drop |= !(lidar_u24(x[0]) < p);
      }
      if (!drop) {
        // mixed pixel: the 4-neighbour of the ideal cast with the largest range jump, up / left / right / down
        double best = 0.0, best_abs = 0.0;
        bool have = false;
        if (r > 0) lidar_partner(hit, t, row - W, T, tt, m.jump, best, best_abs, have);
        if (c > 0) lidar_partner(hit, t, row - 1, T, tt, m.jump, best, best_abs, have);
        if (c < W - 1) lidar_partner(hit, t, row + 1, T, tt, m.jump, best, best_abs, have);
        if (r < H - 1) lidar_partner(hit, t, row + W, T, tt, m.jump, best, best_abs, have);
        const bool mixed = have & (lidar_u24(x[1]) < m.p_mix);
        const double t1 = mixed ? tt + lidar_u24(x[2]) * best : tt;
        // range noise: Irwin-Hall of four uniforms, the sum an integer
        const unsigned long long S = ((unsigned long long)y[0] + y[1]) + ((unsigned long long)y[2] + y[3]);
        const double g = ((double)S * 0x1p-32 - 2.0) * 1.7320508075688772;
        const double t2 = t1 + (m.sigma0 + m.sigma1 * t1) * g;
        const float tf = (float)t2;
        if (__builtin_isfinite(tf) && tf > 0.f) {
          ho = h;
          to = tf;
          kind = mixed ? PN_LIDAR_MIXED : PN_LIDAR_RETURN;
        }
      }
    }
    hit_out[row] = ho;
    t_out[row] = to;
    if (kind_out) kind_out[row] = kind;
  }
}

extern "C" int pn_lidar_sense(const float* tri, int T, const float* poses, int B, const float* dirs, int H, int W, const int32_t* hit,
                              const float* t, uint64_t seed, int frame0, double sigma0, double sigma1, double strength, double range_ref,
                              double min_cos2, double jump, double p_mix, int32_t* hit_out, float* t_out, uint8_t* kind_out,
                              pn_stream stream) {
  const hipStream_t st = S(stream);
  const char* fn = "pn_lidar_sense";
  PN_CHECK_ARG(tri && poses && dirs && hit && t && hit_out && t_out,
               "%s: null pointer (tri, poses, dirs, hit, t, hit_out and t_out are required; kind_out may be NULL)", fn);
  PN_CHECK_ARG((const void*)hit_out != (const void*)hit && (const void*)t_out != (const void*)t,
               "%s: hit_out and t_out must not alias hit and t (a ray reads its neighbours' inputs)", fn);
  PN_CHECK_ARG(B >= 1, "%s: B=%d, at least one frame required", fn, B);
  PN_CHECK_ARG(H >= 1 && W >= 1, "%s: H=%d, W=%d: a raster of at least 1 x 1 required", fn, H, W);
  const long long R = (long long)H * W;
  PN_CHECK_ARG(R <= (1 << 20), "%s: H*W=%lld outside [1, 2^20]", fn, R);
  PN_CHECK_ARG((long long)B * R <= (1ll << 28), "%s: B*H*W=%lld above 2^28", fn, (long long)B * R);
  PN_CHECK_ARG(T >= 1 && T <= (1 << 24), "%s: T=%d outside [1, 2^24]", fn, T);
  PN_CHECK_ARG(frame0 >= 0 && (long long)frame0 + B <= (1ll << 31), "%s: frame0=%d, B=%d: 0 <= frame0 and frame0 + B <= 2^31 required", fn,
               frame0, B);
  PN_CHECK_ARG(sigma0 >= 0.0 && sigma1 >= 0.0, "%s: sigma0=%g, sigma1=%g: both must be >= 0", fn, sigma0, sigma1);
  PN_CHECK_ARG(strength >= 0.0, "%s: strength=%g must be >= 0 (+inf: no detection test)", fn, strength);
  PN_CHECK_ARG(range_ref > 0.0 && range_ref <= 1.7976931348623157e308, "%s: range_ref=%g must be finite and > 0", fn, range_ref);
  PN_CHECK_ARG(min_cos2 >= 0.0 && min_cos2 <= 1.0, "%s: min_cos2=%g outside [0, 1]", fn, min_cos2);
  PN_CHECK_ARG(jump >= 0.0, "%s: jump=%g must be >= 0", fn, jump);
  PN_CHECK_ARG(p_mix >= 0.0 && p_mix <= 1.0, "%s: p_mix=%g outside [0, 1]", fn, p_mix);
  const LidarSensor m = {sigma0, sigma1, strength, range_ref, min_cos2, jump, p_mix};
  const dim3 grid(cdiv((int)R, LS_THREADS), B < LS_MAX_GRID_Y ? B : LS_MAX_GRID_Y);
  hipLaunchKernelGGL(lidar_sense_kernel, grid, dim3(LS_THREADS), 0, st, tri, T, poses, B, dirs, H, W, hit, t,
                     (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), frame0, m, hit_out, t_out, kind_out);
  PN_CHECK_LAUNCH();
  return PN_OK;
}

}  // namespace pn
