// mc.hip -- marching cubes over the SDF volume: an indexed, closed triangle mesh of the level set.
//
// Reference: python/extract_by_mc.py:36-43 calls skimage.measure.marching_cubes on the CPU.  Here the surface is defined by
// a rule (below) from which the 256-case table is GENERATED on the host; outputs are placed by counts and prefix sums, so
// vertex and face order are fully determined and no kernel uses an atomic.
//
// The rule.  A lattice point is inside iff vol < level.  One vertex per lattice edge whose endpoints differ, owned by the
// edge's lower point; vertices ascend by (point linear index, axis).  In a cell, each of the six faces is walked
// counter-clockwise as seen from outside; every maximal run of consecutive inside corners gives one directed segment from the
// crossing where the run ends to the crossing where it begins.  Every crossing edge starts one segment and ends one, so the
// segments link into closed loops; a neighbouring cell walks a shared face the other way and finds the same runs, so shared
// segments cancel and the mesh is closed wherever the surface stays inside the volume.  The loops' right-hand normals point
// toward decreasing values; the table holds the reverse winding ("descent": counter-clockwise seen from the higher-value
// side), each loop cut as a fan.  Faces ascend by cell (the linear index of the cell's origin point), then table order.
//
// Numbering: corner bit c = dx + 2 dy + 4 dz; cube edge = 4 * axis + rank of the edge's lower corner among the four corners
// with d_axis == 0.
//
// Launches (one thread per lattice point, lanes along k, the contiguous axis):
//   k_mc_count       8 corner loads -> case byte and the mask of the point's own crossing edges, kept as a 16-bit code per
//                    point; per-block totals of vertices and triangles
//   k_mc_scan        exclusive scan of the two sets of block totals, one block each, 1024 totals at a time with a carry
//   k_mc_emit_verts  in-block scan of the code's edge counts -> vertex_base of the points that own a vertex, vertex rows
//   k_mc_emit_faces  in-block scan of the table's triangle counts -> faces, each index = vertex_base of the edge's owner +
//                    the rank of the edge's axis among the owner's crossing edges
// The emit kernels read the 2-byte code instead of the volume's eight corners again; only crossing edges reload their two
// samples.  Every loop has a fixed bound, every load and store is guarded by the extent of its array.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <cstring>

#include "common.h"

#pragma clang fp contract(off)

namespace ndjir {

constexpr int MC_BLOCK = 1024;                       // lattice points per block (16 waves)
constexpr int MC_MAX_TRI = 5;                        // triangles per cell, over all 256 cases
constexpr int MC_MAX_DIM = 1 << 15;

// the cube edge between two adjacent corners
static int mc_edge(int c0, int c1) {
  const int d = c0 ^ c1, axis = d == 1 ? 0 : (d == 2 ? 1 : 2), lo = c0 < c1 ? c0 : c1;
  return 4 * axis + ((lo & ((1 << axis) - 1)) | ((lo >> (axis + 1)) << axis));       // bit `axis` of lo (a zero) removed
}

// the lower corner of a cube edge: the inverse of mc_edge
__host__ __device__ __forceinline__ int mc_low_corner(int edge) {
  const int axis = (edge >> 2) & 3, r = edge & 3;
  return (r & ((1 << axis) - 1)) | ((r >> axis) << (axis + 1));
}

struct McPoint {
  int i, j, k;
  bool ex, ey, ez;                                   // the neighbour at +1 along x / y / z exists
};

__device__ __forceinline__ McPoint mc_point(long long p, int Gx, int Gy, int Gz) {
  const unsigned q = (unsigned)p / (unsigned)Gz, k = (unsigned)p - q * (unsigned)Gz;   // p < 2^31
  const unsigned i = q / (unsigned)Gy, j = q - i * (unsigned)Gy;
  return McPoint{(int)i, (int)j, (int)k, (int)i + 1 < Gx, (int)j + 1 < Gy, (int)k + 1 < Gz};
}

// inclusive scan of v over the block's MC_BLOCK threads; returns the sum of the threads before this one plus v
__device__ __forceinline__ int mc_block_scan(int v, int* wsum) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  for (int w = 0; w < MC_BLOCK / 64; ++w)
    if (w < wave) inc += wsum[w];
  return inc;
}

// code[p] = case byte (0 unless p is a cell origin) | mask of p's own crossing edges << 8;
// sums[b] = vertices of block b, sums[nb + b] = triangles of block b
__global__ void __launch_bounds__(MC_BLOCK) k_mc_count(int Gx, int Gy, int Gz, const float* __restrict__ vol, float level,
                                                        const unsigned char* __restrict__ table, unsigned short* __restrict__ code,
                                                        int* __restrict__ sums, int nb) {
  __shared__ unsigned char ntri[256];
  __shared__ int wsum[MC_BLOCK / 64];
  const int tid = threadIdx.x;
  if (tid < 256) ntri[tid] = table[16 * tid];
  __syncthreads();
  const long long N = (long long)Gx * Gy * Gz, p = (long long)blockIdx.x * MC_BLOCK + tid;
  int packed = 0;                                    // vertices | triangles << 16: at most 3072 and 5120 per block
  if (p < N) {
    const McPoint g = mc_point(p, Gx, Gy, Gz);
    const long long sx = (long long)Gy * Gz, sy = Gz;
    unsigned in = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
      // a corner beyond the volume reads the point itself and counts as outside: no branch, so the eight loads go out together
      const bool exists = (!dx || g.ex) && (!dy || g.ey) && (!dz || g.ez);
      const float v = vol[exists ? p + dx * sx + dy * sy + dz : p];
      in |= (exists && v < level ? 1u : 0u) << c;
    }
    const unsigned in0 = in & 1u;
    const unsigned mask = ((g.ex && ((in >> 1) & 1u) != in0) ? 1u : 0u) | ((g.ey && ((in >> 2) & 1u) != in0) ? 2u : 0u) |
                          ((g.ez && ((in >> 4) & 1u) != in0) ? 4u : 0u);
    const unsigned cs = (g.ex && g.ey && g.ez) ? in : 0u;
    code[p] = (unsigned short)(cs | (mask << 8));
    const int nt = ntri[cs] > MC_MAX_TRI ? MC_MAX_TRI : ntri[cs];
    packed = __popc(mask) | (nt << 16);
  }
  for (int o = 32; o > 0; o >>= 1) packed += __shfl_xor(packed, o, 64);
  if ((tid & 63) == 0) wsum[tid >> 6] = packed;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < MC_BLOCK / 64; ++w) s += wsum[w];
    sums[blockIdx.x] = s & 0xffff;
    sums[nb + blockIdx.x] = s >> 16;
  }
}

// Block b scans sums[b * nb .. b * nb + nb) in place to exclusive offsets; counts[b] = the total (capped at INT_MAX),
// counts[2 + b] = 1 if the total exceeds INT_MAX (the offsets are then meaningless).
__global__ void __launch_bounds__(MC_BLOCK) k_mc_scan(int* __restrict__ sums, int nb, int* __restrict__ counts) {
  __shared__ long long wsum[MC_BLOCK / 64];
  __shared__ long long carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int* s = sums + (long long)blockIdx.x * nb;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += MC_BLOCK) {
    const int v = base + tid < nb ? s[base + tid] : 0;
    long long inc = v;
    for (int o = 1; o < 64; o <<= 1) {
      const long long up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    long long before = carry_s;
    for (int w = 0; w < MC_BLOCK / 64; ++w)
      if (w < wave) before += wsum[w];
    if (base + tid < nb) s[base + tid] = (int)(before + inc - v);
    __syncthreads();
    if (tid == MC_BLOCK - 1) carry_s = before + inc;
    __syncthreads();
  }
  if (tid == 0) {
    const long long total = carry_s;
    counts[blockIdx.x] = total > INT_MAX ? INT_MAX : (int)total;
    counts[2 + blockIdx.x] = total > INT_MAX ? 1 : 0;
  }
}

struct McBox {
  float scale[3], mins[3];
};

// vertex_base[p] = number of vertices owned by the points before p, written where p owns one; the rows of p's own vertices.
// Position: index + t along the edge's axis, t = (level - v0) / (v1 - v0); world = pos * scale + mins, a multiply and then an
// add, never an FMA.
__global__ void __launch_bounds__(MC_BLOCK) k_mc_emit_verts(int Gx, int Gy, int Gz, const float* __restrict__ vol, float level,
                                                             const unsigned short* __restrict__ code,
                                                             const int* __restrict__ offsets, McBox box,
                                                             int* __restrict__ vertex_base, float* __restrict__ verts, long long V) {
  __shared__ int wsum[MC_BLOCK / 64];
  const long long N = (long long)Gx * Gy * Gz, p = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
  const unsigned mask = p < N ? (code[p] >> 8) & 7u : 0u;
  const int cnt = __popc(mask);
  long long pos = (long long)offsets[blockIdx.x] + mc_block_scan(cnt, wsum) - cnt;
  if (!mask) return;                                 // (p >= N has no mask) only owners of a crossing edge are looked up
  vertex_base[p] = (int)pos;
  const McPoint g = mc_point(p, Gx, Gy, Gz);
  const long long stride[3] = {(long long)Gy * Gz, Gz, 1};
  const bool exists[3] = {g.ex, g.ey, g.ez};
  const float idx[3] = {(float)g.i, (float)g.j, (float)g.k};
  const float v0 = vol[p];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!((mask >> a) & 1u) || !exists[a]) continue;
    const float v1 = vol[p + stride[a]];
    // plain operators: the file-wide pragma keeps them apart (the __f*_rn wrappers are compiled under the header's
    // contraction mode, and their multiply and add fuse)
    const float t = (level - v0) / (v1 - v0);
    if (pos < V) {
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const float lat = b == a ? idx[b] + t : idx[b];
        const float scaled = lat * box.scale[b];
        verts[pos * 3 + b] = scaled + box.mins[b];
      }
    }
    ++pos;
  }
}

// The faces of the cell at p, from the table row of its case byte.
__global__ void __launch_bounds__(MC_BLOCK) k_mc_emit_faces(int Gx, int Gy, int Gz, const unsigned char* __restrict__ table,
                                                             const unsigned short* __restrict__ code,
                                                             const int* __restrict__ offsets, const int* __restrict__ vertex_base,
                                                             int ascent, int* __restrict__ faces, long long F) {
  __shared__ unsigned char ntri[256];
  __shared__ unsigned int tab[256 * 4];
  __shared__ int wsum[MC_BLOCK / 64];
  const int tid = threadIdx.x;
  if (tid < 256) ntri[tid] = table[16 * tid];
  __syncthreads();
  const long long N = (long long)Gx * Gy * Gz, p = (long long)blockIdx.x * MC_BLOCK + tid;
  const unsigned cs = p < N ? code[p] & 0xffu : 0u;
  const int nt = ntri[cs] > MC_MAX_TRI ? MC_MAX_TRI : ntri[cs];
  long long f = (long long)offsets[blockIdx.x] + mc_block_scan(nt, wsum) - nt;
  int block_total = 0;                               // wsum holds the waves' totals since the scan's barrier
  for (int w = 0; w < MC_BLOCK / 64; ++w) block_total += wsum[w];
  if (!block_total) return;                          // the same for every thread: most blocks hold no surface and skip the table
  tab[tid] = reinterpret_cast<const unsigned int*>(table)[tid];      // 1024 threads x 4 bytes = the table (4-byte aligned)
  __syncthreads();
  if (!nt) return;
  const unsigned char* row = reinterpret_cast<const unsigned char*>(tab) + 16 * cs;
  const long long sx = (long long)Gy * Gz, sy = Gz;
  for (int t = 0; t < MC_MAX_TRI; ++t) {
    if (t >= nt || f >= F) break;
    int v[3];
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int edge = row[1 + 3 * t + e], axis = (edge >> 2) & 3, c = mc_low_corner(edge);
      const long long q = p + (c & 1) * sx + ((c >> 1) & 1) * sy + ((c >> 2) & 1);       // the edge's owner
      v[e] = q < N ? vertex_base[q] + __popc((code[q] >> 8) & ((1u << axis) - 1u)) : 0;
    }
    faces[f * 3] = v[0];
    faces[f * 3 + 1] = ascent ? v[2] : v[1];
    faces[f * 3 + 2] = ascent ? v[1] : v[2];
    ++f;
  }
}

static bool mc_sizes_ok(int Gx, int Gy, int Gz) {
  return Gx >= 2 && Gy >= 2 && Gz >= 2 && Gx <= MC_MAX_DIM && Gy <= MC_MAX_DIM && Gz <= MC_MAX_DIM &&
         (long long)Gx * Gy * Gz <= 0x7fffffffLL;
}

}  // namespace ndjir

extern "C" int ndjir_mc_case_table(unsigned char* host_table) {
  using namespace ndjir;
  if (!host_table) return NDJIR_ERR_ARG;
  static const int ccw[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
  for (int cs = 0; cs < 256; ++cs) {
    unsigned char* row = host_table + 16 * cs;
    std::memset(row, 0, 16);
    int next[12];
    for (int e = 0; e < 12; ++e) next[e] = -1;
    for (int a = 0; a < 3; ++a) {
      const int u = (a + 1) % 3, v = (a + 2) % 3;      // e_u x e_v = e_a
      for (int side = 0; side < 2; ++side) {
        int w[4], ins[4], n_in = 0;                    // the face's corners counter-clockwise about its outward normal
        for (int n = 0; n < 4; ++n) {
          const int pu = side ? ccw[n][0] : ccw[n][1], pv = side ? ccw[n][1] : ccw[n][0];
          w[n] = (side << a) | (pu << u) | (pv << v);
          ins[n] = (cs >> w[n]) & 1;
          n_in += ins[n];
        }
        if (n_in == 0 || n_in == 4) continue;
        for (int s = 0; s < 4; ++s) {
          if (!ins[s] || ins[(s + 3) & 3]) continue;   // a run of inside corners begins at s ...
          int e = s;
          for (int step = 0; step < 3 && ins[(e + 1) & 3]; ++step) e = (e + 1) & 3;   // ... and ends at e
          next[mc_edge(w[e], w[(e + 1) & 3])] = mc_edge(w[(s + 3) & 3], w[s]);
        }
      }
    }
    bool seen[12] = {};
    int nt = 0;
    for (int start = 0; start < 12; ++start) {
      if (next[start] < 0 || seen[start]) continue;
      int loop[12], n = 0;
      for (int e = start; n < 12 && e >= 0 && !seen[e]; e = next[e]) {
        seen[e] = true;
        loop[n++] = e;
      }
      for (int m = 1; m + 1 < n; ++m) {                // a fan in the reverse of the loop's direction ("descent")
        if (nt == MC_MAX_TRI) return NDJIR_ERR_CAPACITY;
        row[1 + 3 * nt] = (unsigned char)loop[0];
        row[2 + 3 * nt] = (unsigned char)loop[m + 1];
        row[3 + 3 * nt] = (unsigned char)loop[m];
        ++nt;
      }
    }
    row[0] = (unsigned char)nt;
  }
  return NDJIR_OK;
}

extern "C" int ndjir_mc_count(int Gx, int Gy, int Gz, const float* vol, float level, const unsigned char* table,
                              unsigned short* code, int* block_sums, int* counts, hipStream_t stream) {
  using namespace ndjir;
  if (!mc_sizes_ok(Gx, Gy, Gz) || !vol || !table || !code || !block_sums || !counts) return NDJIR_ERR_ARG;
  const long long N = (long long)Gx * Gy * Gz;
  const int nb = (int)((N + MC_BLOCK - 1) / MC_BLOCK);
  hipLaunchKernelGGL(k_mc_count, dim3((unsigned)nb), dim3(MC_BLOCK), 0, stream, Gx, Gy, Gz, vol, level, table, code, block_sums, nb);
  hipLaunchKernelGGL(k_mc_scan, dim3(2), dim3(MC_BLOCK), 0, stream, block_sums, nb, counts);
  return ndjir_check_launch();
}

extern "C" int ndjir_mc_emit(int Gx, int Gy, int Gz, const float* vol, float level, const unsigned char* table,
                             const unsigned short* code, const int* block_offsets, const float* scale, const float* mins, int ascent,
                             int* vertex_base, float* verts, long long V, int* faces, long long F, hipStream_t stream) {
  using namespace ndjir;
  if (!mc_sizes_ok(Gx, Gy, Gz) || !vol || !table || !code || !block_offsets || !scale || !mins || !vertex_base) return NDJIR_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(table) & 3u) return NDJIR_ERR_ARG;
  if (V < 0 || F < 0 || V > 0x7fffffffLL || F > 0x7fffffffLL || (V > 0 && !verts) || (F > 0 && !faces)) return NDJIR_ERR_ARG;
  const long long N = (long long)Gx * Gy * Gz;
  const int nb = (int)((N + MC_BLOCK - 1) / MC_BLOCK);
  McBox box;
  for (int a = 0; a < 3; ++a) {
    box.scale[a] = scale[a];
    box.mins[a] = mins[a];
  }
  hipLaunchKernelGGL(k_mc_emit_verts, dim3((unsigned)nb), dim3(MC_BLOCK), 0, stream, Gx, Gy, Gz, vol, level, code, block_offsets, box,
                     vertex_base, verts, V);
  if (F > 0)
    hipLaunchKernelGGL(k_mc_emit_faces, dim3((unsigned)nb), dim3(MC_BLOCK), 0, stream, Gx, Gy, Gz, table, code, block_offsets + nb,
                       (const int*)vertex_base, ascent, faces, F);
  return ndjir_check_launch();
}
