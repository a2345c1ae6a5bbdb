// chamfer.hip -- the DTU Chamfer evaluation of an extracted mesh (python/evaluate_chamfer_dtumvs.py:84-175).
//
// The reference samples the triangles in a process pool (`sample_single_tri`, :32-41, :92-108), thins the cloud with a
// kd-tree radius query and a sequential Python loop (:124-133), filters it by the observation mask (:141-149) and the ground
// plane (:166-170) in numpy, and takes two kd-tree nearest-neighbour passes (:158-174).  Here:
//   k_ch_tri_rows, k_ch_row_counts, k_ch_emit_points   sampling: rows (n1 + 1) per triangle, kept candidates per row, the
//                                                      points; every order comes from prefix sums (k_ch_block_sums,
//                                                      k_ch_scan_totals, k_ch_offsets)
//   k_ch_cell_keys                                     the int64 cell key of a point in a uniform grid
//   k_ch_thin_round                                    one round of the greedy thinning as a parallel iteration
//   k_ch_mask_points, k_ch_above_plane                 the two filters
//   k_ch_nearest                                       the nearest target closer than max_dist, shell by shell
// All coordinate arithmetic is fp64, one operation at a time in the order of the reference's numpy expressions (no
// contraction: the file-wide pragma), so every result but the nearest distance's last bit is the reference's.  A grid is
// sparse: the points sorted by key (the caller sorts), a cell is found by a binary search for its key, the cells
// (ix, iy, z0 .. z1) are one contiguous run.  No kernel waits for another block; every loop is bounded by its input.
#include <hip/hip_runtime.h>

#include <climits>

#include "common.h"

#pragma clang fp contract(off)

namespace ndjir {

constexpr int CH_THREADS = 256;
constexpr int CH_SCAN = 1024;                        // elements per block of the scan kernels (16 waves)
constexpr int CH_MAX_N = 32767;                      // largest n1 or n2 of one triangle (include/ndjir_hip.h)
constexpr long long CH_MAX_DIM = 1LL << 20;          // cells per axis: a key fits 60 bits
constexpr double CH_GUARD = 1.0 / 1048576.0;         // 2^-20: slack for the rounding of a cell coordinate (below)
constexpr double CH_FAR_CELL = 1099511627776.0;      // 2^40: a query's cell coordinate is clamped to +-this
constexpr int CH_MAX_SHELLS = 66;                    // max_dist / h <= 64, plus the two shells of slack

constexpr unsigned char TH_UNDECIDED = 0, TH_KEPT = 1, TH_DROPPED = 2;

struct ChGrid {                                      // origin, cell size, cells per axis
  double o[3], h;
  long long n[3];
};

static inline unsigned ch_blocks(long long n, int per) { return (unsigned)((n + per - 1) / per); }

// ---- prefix sums -----------------------------------------------------------------------------------------------------------
// offsets[i] = vals[0] + ... + vals[i - 1] in three launches: block totals, a one-block scan of the totals (64-bit carry:
// counts[0] = the total capped at INT_MAX, counts[1] = 1 if it exceeds INT_MAX), the in-block prefix added to the block's.
__device__ __forceinline__ int ch_block_scan(int v, int* wsum) {       // inclusive, over the block's CH_SCAN threads
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  for (int w = 0; w < CH_SCAN / 64; ++w)
    if (w < wave) inc += wsum[w];
  return inc;
}

__global__ void __launch_bounds__(CH_SCAN) k_ch_block_sums(long long n, const int* __restrict__ vals, int* __restrict__ sums) {
  __shared__ int wsum[CH_SCAN / 64];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * CH_SCAN + tid;
  int v = i < n ? vals[i] : 0;                       // a block's total is at most 1024 * 32768 = 2^25
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < CH_SCAN / 64; ++w) s += wsum[w];
    sums[blockIdx.x] = s;
  }
}

__global__ void __launch_bounds__(CH_SCAN) k_ch_scan_totals(int* __restrict__ sums, int nb, int* __restrict__ counts) {
  __shared__ long long wsum[CH_SCAN / 64];
  __shared__ long long carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += CH_SCAN) {
    const int v = base + tid < nb ? sums[base + tid] : 0;
    long long inc = v;
    for (int o = 1; o < 64; o <<= 1) {
      const long long up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long before = carry_s;
    for (int w = 0; w < CH_SCAN / 64; ++w)
      if (w < wave) before += wsum[w];
    if (base + tid < nb) sums[base + tid] = (int)(before + inc - v);
    __syncthreads();
    if (tid == CH_SCAN - 1) carry_s = before + inc;
    __syncthreads();
  }
  if (tid == 0) {
    const long long total = carry_s;
    counts[0] = total > INT_MAX ? INT_MAX : (int)total;
    counts[1] = total > INT_MAX ? 1 : 0;
  }
}

__global__ void __launch_bounds__(CH_SCAN) k_ch_offsets(long long n, const int* __restrict__ vals, const int* __restrict__ block_offsets,
                                                     int* __restrict__ offsets) {
  __shared__ int wsum[CH_SCAN / 64];
  const long long i = (long long)blockIdx.x * CH_SCAN + threadIdx.x;
  const int v = i < n ? vals[i] : 0;
  const int inc = ch_block_scan(v, wsum);
  if (i < n) offsets[i] = block_offsets[blockIdx.x] + inc - v;
}

// ---- triangle sampling -----------------------------------------------------------------------------------------------------
struct ChTri {
  double p0[3], v1[3], v2[3];
};

// :86, :92-93; false if a vertex index lies outside [0, N)
__device__ __forceinline__ bool ch_triangle(const double* __restrict__ verts, long long N, const int* __restrict__ faces, long long t,
                                            ChTri& tr) {
  const int a = faces[t * 3], b = faces[t * 3 + 1], c = faces[t * 3 + 2];
  if (a < 0 || b < 0 || c < 0 || a >= N || b >= N || c >= N) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    tr.p0[k] = verts[3LL * a + k];
    tr.v1[k] = verts[3LL * b + k] - tr.p0[k];
    tr.v2[k] = verts[3LL * c + k] - tr.p0[k];
  }
  return true;
}

// np.linalg.norm(v, axis=-1): the squares summed left to right
__device__ __forceinline__ double ch_norm3(double x, double y, double z) { return sqrt(x * x + y * y + z * z); }

// rows[t] = n1 + 1 (0: the triangle yields nothing), n2s[t] = n2 (:94-103).  flags[0]: some n1 or n2 exceeds CH_MAX_N or is
// not a number; flags[1]: a vertex index out of range.
__global__ void __launch_bounds__(CH_THREADS) k_ch_tri_rows(long long N, const double* __restrict__ verts, long long F,
                                                         const int* __restrict__ faces, double thresh, int* __restrict__ rows,
                                                         int* __restrict__ n2s, int* __restrict__ flags) {
  const long long t = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
  if (t >= F) return;
  int r = 0, m = 0;
  ChTri tr;
  if (!ch_triangle(verts, N, faces, t, tr)) {
    atomicOr(flags + 1, 1);
  } else {
    const double l1 = ch_norm3(tr.v1[0], tr.v1[1], tr.v1[2]), l2 = ch_norm3(tr.v2[0], tr.v2[1], tr.v2[2]);
    const double cx = tr.v1[1] * tr.v2[2] - tr.v1[2] * tr.v2[1];      // np.cross
    const double cy = tr.v1[2] * tr.v2[0] - tr.v1[0] * tr.v2[2];
    const double cz = tr.v1[0] * tr.v2[1] - tr.v1[1] * tr.v2[0];
    const double area2 = ch_norm3(cx, cy, cz);
    if (area2 > 0.0) {
      const double thr = thresh * sqrt(l1 * l2 / area2);
      const double n1 = floor(l1 / thr), n2 = floor(l2 / thr);
      if (!(n1 <= (double)CH_MAX_N) || !(n2 <= (double)CH_MAX_N) || !(n1 >= 0.0) || !(n2 >= 0.0)) {
        atomicOr(flags, 1);
      } else if (n1 >= 1.0 && n2 >= 1.0) {           // n == 0 divides by 1e-7: k = 5e6, nothing passes k0 + k1 < 1
        r = (int)n1 + 1;
        m = (int)n2;
      }
    }
  }
  rows[t] = r;
  n2s[t] = m;
}

// (i + 0.5) / max(n, 1e-7) (:34-37)
__device__ __forceinline__ double ch_k(int i, int n) { return ((double)i + 0.5) / fmax((double)n, 1e-7); }

// The last triangle whose first row is <= r: triangles without rows share their successor's offset, so this is r's owner.
__device__ __forceinline__ int ch_row_owner(const int* __restrict__ tri_row_off, long long F, int r) {
  long long lo = 0, hi = F;                          // the first t with tri_row_off[t] > r
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (tri_row_off[mid] <= r) lo = mid + 1; else hi = mid;
  }
  return (int)(lo - 1);
}

// Row i of triangle t keeps the candidates j with k0 + k1(j) < 1 in fp64 (:39).  k1 and the rounded sum do not decrease
// with j, so they are j = 0 .. m - 1, and m comes from a bisection with the reference's own expression as the test.
__global__ void __launch_bounds__(CH_THREADS) k_ch_row_counts(long long F, const int* __restrict__ rows, const int* __restrict__ n2s,
                                                           const int* __restrict__ tri_row_off, long long R, int* __restrict__ row_tri,
                                                           int* __restrict__ row_cnt) {
  const long long r = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
  if (r >= R) return;
  const int t = ch_row_owner(tri_row_off, F, (int)r);
  const int i = (int)r - tri_row_off[t], n1 = rows[t] - 1, n2 = n2s[t];
  const double k0 = ch_k(i, n1);
  int lo = 0, hi = n2 + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (k0 + ch_k(mid, n2) < 1.0) lo = mid + 1; else hi = mid;
  }
  row_tri[r] = t;
  row_cnt[r] = lo;
}

// q = (v1 k0 + v2 k1) + p0 (:40), the rows in (triangle, i) order, j ascending inside a row
__global__ void __launch_bounds__(CH_THREADS) k_ch_emit_points(long long N, const double* __restrict__ verts, const int* __restrict__ faces,
                                                            const int* __restrict__ rows, const int* __restrict__ n2s,
                                                            const int* __restrict__ tri_row_off, long long R,
                                                            const int* __restrict__ row_tri, const int* __restrict__ row_cnt,
                                                            const int* __restrict__ row_pt_off, long long S, double* __restrict__ points) {
  const long long r = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
  if (r >= R) return;
  const int m = row_cnt[r];
  if (m <= 0) return;
  const int t = row_tri[r];
  ChTri tr;
  if (!ch_triangle(verts, N, faces, t, tr)) return;
  const int i = (int)r - tri_row_off[t], n1 = rows[t] - 1, n2 = n2s[t];
  const double k0 = ch_k(i, n1);
  long long pos = row_pt_off[r];
  for (int j = 0; j < m && pos < S; ++j, ++pos) {
    const double k1 = ch_k(j, n2);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double a = tr.v1[k] * k0, b = tr.v2[k] * k1;
      points[pos * 3 + k] = (a + b) + tr.p0[k];
    }
  }
}

// ---- the sparse grid ---------------------------------------------------------------------------------------------------------
// Cell coordinate along axis a: f = (p - origin) / h, cell = floor(f); key = (cx ny + cy) nz + cz.
__device__ __forceinline__ double ch_cell_f(const ChGrid& g, int a, double p) { return (p - g.o[a]) / g.h; }

__device__ __forceinline__ long long ch_clamp_cell(double f, long long n) {
  if (!(f >= 0.0)) return 0;                         // NaN too
  const double c = floor(f);
  return c >= (double)n ? n - 1 : (long long)c;
}

__global__ void __launch_bounds__(CH_THREADS) k_ch_cell_keys(long long N, const double* __restrict__ pts, ChGrid g,
                                                          long long* __restrict__ keys) {
  const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
  if (i >= N) return;
  long long c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) c[a] = ch_clamp_cell(ch_cell_f(g, a, pts[i * 3 + a]), g.n[a]);
  keys[i] = (c[0] * g.n[1] + c[1]) * g.n[2] + c[2];
}

// the first j with keys[j] >= key
__device__ __forceinline__ long long ch_lower_bound(const long long* __restrict__ keys, long long n, long long key) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- thinning ----------------------------------------------------------------------------------------------------------------
// The reference keeps point i iff no kept point earlier in the (shuffled) order lies within thresh (:128-132): the
// lexicographically first maximal independent set.  One round, from the previous round's states only: an undecided point
// with a kept earlier neighbour is dropped; one whose earlier neighbours are all dropped is kept; otherwise it waits.  The
// earliest undecided point is always decided, so the count of undecided points falls every round.
// The points are in key order (cell = thresh); rank[i] = position of point i in the processing order.  A neighbour within
// thresh lies at most one cell away per axis -- up to the rounding of f, which is far below CH_GUARD of a cell: a point that
// close to a cell wall also looks two cells that way.
__global__ void __launch_bounds__(CH_THREADS) k_ch_thin_round(long long N, const double* __restrict__ pts, const long long* __restrict__ keys,
                                                           const int* __restrict__ rank, ChGrid g, double thresh,
                                                           const unsigned char* __restrict__ in, unsigned char* __restrict__ out,
                                                           int* __restrict__ undecided) {
  const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
  unsigned char s = TH_KEPT;
  if (i < N) {
    s = in[i];
    if (s == TH_UNDECIDED) {
      const double p[3] = {pts[i * 3], pts[i * 3 + 1], pts[i * 3 + 2]};
      const int my = rank[i];
      const double t2 = thresh * thresh;
      long long lo[3], hi[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double f = ch_cell_f(g, a, p[a]);
        const long long c = ch_clamp_cell(f, g.n[a]);
        const double frac = f - (double)c;
        lo[a] = c - 1 - (frac < CH_GUARD ? 1 : 0);
        hi[a] = c + 1 + (frac > 1.0 - CH_GUARD ? 1 : 0);
        if (lo[a] < 0) lo[a] = 0;
        if (hi[a] > g.n[a] - 1) hi[a] = g.n[a] - 1;
      }
      bool blocked = false, dropped = false;
      for (long long ix = lo[0]; ix <= hi[0] && !dropped; ++ix)
        for (long long iy = lo[1]; iy <= hi[1] && !dropped; ++iy) {
          const long long base = (ix * g.n[1] + iy) * g.n[2], last = base + hi[2];
          for (long long j = ch_lower_bound(keys, N, base + lo[2]); j < N && keys[j] <= last; ++j) {
            if (rank[j] >= my) continue;             // later in the order, or the point itself
            const unsigned char sj = in[j];
            if (sj == TH_DROPPED) continue;
            const double dx = pts[j * 3] - p[0], dy = pts[j * 3 + 1] - p[1], dz = pts[j * 3 + 2] - p[2];
            if (!(dx * dx + dy * dy + dz * dz <= t2)) continue;
            if (sj == TH_KEPT) {
              dropped = true;
              break;
            }
            blocked = true;
          }
        }
      s = dropped ? TH_DROPPED : (blocked ? TH_UNDECIDED : TH_KEPT);
    }
    out[i] = s;
  }
  const unsigned long long b = __ballot(s == TH_UNDECIDED);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(undecided, __popcll(b));
}

// ---- observation mask and ground plane -------------------------------------------------------------------------------------
struct ChMask {
  double lo[3], hi[3], bb0[3], res;
  int n[3];
};

// :142, :145-148.  lo = BB0 - patch and hi = BB1 + 2 patch arrive as the reference rounds them (fp32 arithmetic on the host).
__global__ void __launch_bounds__(CH_THREADS) k_ch_mask_points(long long N, const double* __restrict__ pts, ChMask m,
                                                            const unsigned char* __restrict__ mask, unsigned char* __restrict__ in_bb,
                                                            unsigned char* __restrict__ in_obs) {
  const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
  if (i >= N) return;
  bool inb = true, ing = true;
  long long cell = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double p = pts[i * 3 + a];
    inb = inb && p >= m.lo[a] && p < m.hi[a];
    const double gidx = rint((p - m.bb0[a]) / m.res);                 // np.around: half to even
    const bool ok = gidx >= 0.0 && gidx < (double)m.n[a];
    ing = ing && ok;
    cell = cell * m.n[a] + (ok ? (long long)gidx : 0);
  }
  in_bb[i] = inb ? 1 : 0;
  in_obs[i] = (inb && ing && mask[cell] != 0) ? 1 : 0;
}

// :168-169: (P * [x, y, z, 1]).sum(-1) > 0, the four products summed left to right
__global__ void __launch_bounds__(CH_THREADS) k_ch_above_plane(long long N, const double* __restrict__ pts, double p0, double p1, double p2,
                                                            double p3, unsigned char* __restrict__ above) {
  const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
  if (i >= N) return;
  const double s = p0 * pts[i * 3] + p1 * pts[i * 3 + 1] + p2 * pts[i * 3 + 2] + p3 * 1.0;
  above[i] = s > 0.0 ? 1 : 0;
}

// ---- bounded nearest neighbour ---------------------------------------------------------------------------------------------
struct ChBest {
  double d2;
  long long j;
};

// the targets of cells (ix, iy, z0 .. z1), z0 <= z1 inside the grid
__device__ __forceinline__ void ch_probe(const double* __restrict__ pts, const long long* __restrict__ keys, long long T, const ChGrid& g,
                                         long long ix, long long iy, long long z0, long long z1, const double* q, ChBest& best) {
  const long long base = (ix * g.n[1] + iy) * g.n[2], last = base + z1;
  for (long long j = ch_lower_bound(keys, T, base + z0); j < T && keys[j] <= last; ++j) {
    const double dx = pts[j * 3] - q[0], dy = pts[j * 3 + 1] - q[1], dz = pts[j * 3 + 2] - q[2];
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (d2 < best.d2) {
      best.d2 = d2;
      best.j = j;
    }
  }
}

// a lower bound of |t - q| along one axis for a target d cells away: (|d| - 1) h, less the rounding of the cell coordinates
__device__ __forceinline__ double ch_gap(long long d, double h) {
  const long long a = d < 0 ? -d : d;
  return a <= 1 ? 0.0 : (double)(a - 1) * h * (1.0 - CH_GUARD);
}

// One query per lane.  Shell s = the cells at Chebyshev distance s from the query's cell; nothing in it is closer than
// ch_gap(s), so the search ends once the best distance is no greater than that, or the shell lies beyond max_dist.  Inside a
// shell a column (ix, iy) is skipped when its own gap already rules it out.
__global__ void __launch_bounds__(CH_THREADS) k_ch_nearest(long long Q, const double* __restrict__ queries, long long T,
                                                        const double* __restrict__ pts, const long long* __restrict__ keys, ChGrid g,
                                                        double max_dist, double* __restrict__ dist, int* __restrict__ idx) {
  const long long i = (long long)blockIdx.x * CH_THREADS + threadIdx.x;
  if (i >= Q) return;
  const double q[3] = {queries[i * 3], queries[i * 3 + 1], queries[i * 3 + 2]};
  const double inf = __builtin_huge_val();
  ChBest best{inf, -1};
  long long c[3];
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double f = ch_cell_f(g, a, q[a]);
    ok = ok && f == f;
    f = fmin(fmax(f, -CH_FAR_CELL), CH_FAR_CELL);
    c[a] = (long long)floor(f);
  }
  const double md2 = max_dist * max_dist * (1.0 + CH_GUARD);
  for (int s = 0; ok && s < CH_MAX_SHELLS; ++s) {
    const double lb = ch_gap(s, g.h);
    if (lb >= max_dist || best.d2 <= lb * lb) break;
    const long long x0 = c[0] - s < 0 ? 0 : c[0] - s, x1 = c[0] + s > g.n[0] - 1 ? g.n[0] - 1 : c[0] + s;
    const long long y0 = c[1] - s < 0 ? 0 : c[1] - s, y1 = c[1] + s > g.n[1] - 1 ? g.n[1] - 1 : c[1] + s;
    const long long zlo = c[2] - s, zhi = c[2] + s;
    const long long z0 = zlo < 0 ? 0 : zlo, z1 = zhi > g.n[2] - 1 ? g.n[2] - 1 : zhi;
    for (long long ix = x0; ix <= x1; ++ix) {
      const long long ax = ix - c[0] < 0 ? c[0] - ix : ix - c[0];
      const double gx = ch_gap(ax, g.h);
      for (long long iy = y0; iy <= y1; ++iy) {
        const long long ay = iy - c[1] < 0 ? c[1] - iy : iy - c[1];
        const double gy = ch_gap(ay, g.h), col2 = gx * gx + gy * gy;
        if (col2 > md2 || best.d2 <= col2) continue;
        if (ax == s || ay == s) {                    // the shell's side walls: the whole column
          if (z0 <= z1) ch_probe(pts, keys, T, g, ix, iy, z0, z1, q, best);
        } else {                                     // its floor and its ceiling
          if (zlo >= 0 && zlo < g.n[2]) ch_probe(pts, keys, T, g, ix, iy, zlo, zlo, q, best);
          if (zhi >= 0 && zhi < g.n[2]) ch_probe(pts, keys, T, g, ix, iy, zhi, zhi, q, best);
        }
      }
    }
  }
  const double d = best.j >= 0 ? sqrt(best.d2) : inf;
  const bool found = d < max_dist;
  dist[i] = found ? d : inf;
  idx[i] = found ? (int)best.j : -1;
}

static bool ch_grid(const double* origin, double h, const long long* dims, ChGrid& g) {
  if (!origin || !dims || !(h > 0.0) || !(h < __builtin_huge_val())) return false;
  g.h = h;
  for (int a = 0; a < 3; ++a) {
    if (!(origin[a] == origin[a]) || dims[a] < 1 || dims[a] > CH_MAX_DIM) return false;
    g.o[a] = origin[a];
    g.n[a] = dims[a];
  }
  return true;
}

}  // namespace ndjir

extern "C" int ndjir_chamfer_scan(long long n, const int* vals, int* offsets, int* workspace, int* counts, hipStream_t stream) {
  using namespace ndjir;
  if (n < 0 || n > 0x7fffffffLL || !counts) return NDJIR_ERR_ARG;
  if (hipMemsetAsync(counts, 0, 2 * sizeof(int), stream) != hipSuccess) return NDJIR_ERR_LAUNCH;
  if (n == 0) return NDJIR_OK;
  if (!vals || !offsets || !workspace) return NDJIR_ERR_ARG;
  const unsigned nb = ch_blocks(n, CH_SCAN);
  hipLaunchKernelGGL(k_ch_block_sums, dim3(nb), dim3(CH_SCAN), 0, stream, n, vals, workspace);
  hipLaunchKernelGGL(k_ch_scan_totals, dim3(1), dim3(CH_SCAN), 0, stream, workspace, (int)nb, counts);
  hipLaunchKernelGGL(k_ch_offsets, dim3(nb), dim3(CH_SCAN), 0, stream, n, vals, (const int*)workspace, offsets);
  return ndjir_check_launch();
}

extern "C" int ndjir_chamfer_tri_rows(long long N, const double* verts, long long F, const int* faces, double thresh, int* rows, int* n2s,
                                      int* flags, hipStream_t stream) {
  using namespace ndjir;
  if (N < 0 || N > 0x7fffffffLL || F < 0 || F > 0x7fffffffLL / 3 || !(thresh > 0.0) || !flags) return NDJIR_ERR_ARG;
  if (hipMemsetAsync(flags, 0, 2 * sizeof(int), stream) != hipSuccess) return NDJIR_ERR_LAUNCH;
  if (F == 0) return NDJIR_OK;
  if (!faces || !rows || !n2s || (N > 0 && !verts)) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(k_ch_tri_rows, dim3(ch_blocks(F, CH_THREADS)), dim3(CH_THREADS), 0, stream, N, verts, F, faces, thresh, rows, n2s, flags);
  return ndjir_check_launch();
}

extern "C" int ndjir_chamfer_row_counts(long long F, const int* rows, const int* n2s, const int* tri_row_off, long long R, int* row_tri,
                                        int* row_cnt, hipStream_t stream) {
  using namespace ndjir;
  if (F < 0 || F > 0x7fffffffLL / 3 || R < 0 || R > 0x7fffffffLL) return NDJIR_ERR_ARG;
  if (R == 0) return NDJIR_OK;
  if (F == 0 || !rows || !n2s || !tri_row_off || !row_tri || !row_cnt) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(k_ch_row_counts, dim3(ch_blocks(R, CH_THREADS)), dim3(CH_THREADS), 0, stream, F, rows, n2s, tri_row_off, R, row_tri,
                     row_cnt);
  return ndjir_check_launch();
}

extern "C" int ndjir_chamfer_emit_points(long long N, const double* verts, const int* faces, const int* rows, const int* n2s,
                                         const int* tri_row_off, long long R, const int* row_tri, const int* row_cnt,
                                         const int* row_pt_off, long long S, double* points, hipStream_t stream) {
  using namespace ndjir;
  if (N < 0 || N > 0x7fffffffLL || R < 0 || R > 0x7fffffffLL || S < 0 || S > 0x7fffffffLL) return NDJIR_ERR_ARG;
  if (R == 0 || S == 0) return NDJIR_OK;
  if (!verts || !faces || !rows || !n2s || !tri_row_off || !row_tri || !row_cnt || !row_pt_off || !points) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(k_ch_emit_points, dim3(ch_blocks(R, CH_THREADS)), dim3(CH_THREADS), 0, stream, N, verts, faces, rows, n2s, tri_row_off, R,
                     row_tri, row_cnt, row_pt_off, S, points);
  return ndjir_check_launch();
}

extern "C" int ndjir_chamfer_cell_keys(long long N, const double* points, const double* origin, double h, const long long* dims,
                                       long long* keys, hipStream_t stream) {
  using namespace ndjir;
  ChGrid g;
  if (N < 0 || N > 0x7fffffffLL || !ch_grid(origin, h, dims, g)) return NDJIR_ERR_ARG;
  if (N == 0) return NDJIR_OK;
  if (!points || !keys) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(k_ch_cell_keys, dim3(ch_blocks(N, CH_THREADS)), dim3(CH_THREADS), 0, stream, N, points, g, keys);
  return ndjir_check_launch();
}

extern "C" int ndjir_chamfer_thin_round(long long N, const double* points, const long long* keys, const int* rank, const double* origin,
                                        double thresh, const long long* dims, const unsigned char* state_in, unsigned char* state_out,
                                        int* undecided, hipStream_t stream) {
  using namespace ndjir;
  ChGrid g;
  if (N < 0 || N > 0x7fffffffLL || !ch_grid(origin, thresh, dims, g) || !undecided) return NDJIR_ERR_ARG;
  if (hipMemsetAsync(undecided, 0, sizeof(int), stream) != hipSuccess) return NDJIR_ERR_LAUNCH;
  if (N == 0) return NDJIR_OK;
  if (!points || !keys || !rank || !state_in || !state_out || state_in == state_out) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(k_ch_thin_round, dim3(ch_blocks(N, CH_THREADS)), dim3(CH_THREADS), 0, stream, N, points, keys, rank, g, thresh, state_in,
                     state_out, undecided);
  return ndjir_check_launch();
}

extern "C" int ndjir_chamfer_mask_points(long long N, const double* points, const double* lo, const double* hi, const double* bb0,
                                         double res, const int* dims, const unsigned char* mask, unsigned char* in_bb,
                                         unsigned char* in_obs, hipStream_t stream) {
  using namespace ndjir;
  if (N < 0 || N > 0x7fffffffLL || !lo || !hi || !bb0 || !dims || !(res > 0.0)) return NDJIR_ERR_ARG;
  ChMask m;
  m.res = res;
  for (int a = 0; a < 3; ++a) {
    if (dims[a] < 1) return NDJIR_ERR_ARG;
    m.lo[a] = lo[a];
    m.hi[a] = hi[a];
    m.bb0[a] = bb0[a];
    m.n[a] = dims[a];
  }
  if (N == 0) return NDJIR_OK;
  if (!points || !mask || !in_bb || !in_obs) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(k_ch_mask_points, dim3(ch_blocks(N, CH_THREADS)), dim3(CH_THREADS), 0, stream, N, points, m, mask, in_bb, in_obs);
  return ndjir_check_launch();
}

extern "C" int ndjir_chamfer_above_plane(long long N, const double* points, const double* plane, unsigned char* above,
                                         hipStream_t stream) {
  using namespace ndjir;
  if (N < 0 || N > 0x7fffffffLL || !plane) return NDJIR_ERR_ARG;
  if (N == 0) return NDJIR_OK;
  if (!points || !above) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(k_ch_above_plane, dim3(ch_blocks(N, CH_THREADS)), dim3(CH_THREADS), 0, stream, N, points, plane[0], plane[1], plane[2],
                     plane[3], above);
  return ndjir_check_launch();
}

extern "C" int ndjir_chamfer_nearest(long long Q, const double* queries, long long T, const double* targets, const long long* keys,
                                     const double* origin, double h, const long long* dims, double max_dist, double* dist, int* idx,
                                     hipStream_t stream) {
  using namespace ndjir;
  ChGrid g;
  if (Q < 0 || Q > 0x7fffffffLL || T < 1 || T > 0x7fffffffLL || !ch_grid(origin, h, dims, g)) return NDJIR_ERR_ARG;
  if (!(max_dist > 0.0) || !(max_dist <= 64.0 * h)) return NDJIR_ERR_ARG;
  if (Q == 0) return NDJIR_OK;
  if (!queries || !targets || !keys || !dist || !idx) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(k_ch_nearest, dim3(ch_blocks(Q, CH_THREADS)), dim3(CH_THREADS), 0, stream, Q, queries, T, targets, keys, g, max_dist, dist,
                     idx);
  return ndjir_check_launch();
}
