// trim.hip -- trimming an extracted mesh by the camera masks and splitting it into connected components.
//
// Reference: python/extract_by_mc.py:77-128.  `clean_points_by_mask` (:77-102) dilates every mask with a 101 x 101 ellipse
// (cv2 on the CPU), projects every vertex into every view in numpy and looks the pixel up in the dilated mask with a
// one-pixel frame of ones; `create_trimmed_meshes` (:105-128) drops the vertices that fall outside any view's mask and the
// faces that lose a vertex, re-indexes, and splits the rest with trimesh (faces connected through shared edges).  Every
// result is an integer, so the kernels below reproduce the reference exactly:
//   k_row_dist, k_dilate      the dilation as a row pass (distance to the nearest set pixel of the row) and a column pass
//   k_points_in_masks         the projection in fp64, operation by operation, one lane per vertex
//   k_flag_count, k_scan_totals, k_flag_emit   a stable stream compaction from wave ballots (vertices and faces)
//   k_cc_init, k_cc_edges, k_cc_flatten        edge matching in an open-addressing hash table + lock-free union-find
// Every loop that depends on another thread's progress is bounded and reports through a status word.
#include <hip/hip_runtime.h>

#include "common.h"

#pragma clang fp contract(off)

namespace ndjir {

constexpr int TR_THREADS = 256;
constexpr int TR_MAX_R = 127;                      // largest dilation radius: distances and half-widths fit a byte
constexpr int TR_TILE = 64;                        // k_dilate: 64 x 64 output pixels per block
constexpr int TR_SCAN = 1024;                      // elements per block of the compaction kernels (16 waves)
constexpr unsigned char TR_FAR = 255;              // "no set pixel within reach in this row"

struct HalfTable {
  unsigned char h[2 * TR_MAX_R + 2];               // row half-widths of the structuring element, h[dy + r]
};

// ---- mask dilation ---------------------------------------------------------------------------------------------------------
// dist[m][y][x] = horizontal distance from (y, x) to the nearest set pixel (mask >= 0.5) of row y, TR_FAR beyond 127.
// One block per 256-pixel row segment: the set bits of columns x0 - 128 ... x0 + 383 as eight 64-bit ballots in LDS, then a
// bit scan to either side per pixel.
__global__ void __launch_bounds__(TR_THREADS) k_row_dist(int H, int W, const float* __restrict__ masks,
                                                         unsigned char* __restrict__ dist) {
  __shared__ unsigned long long bits[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = blockIdx.x * TR_THREADS, y = blockIdx.y;
  const long long row = ((long long)blockIdx.z * H + y) * W;
  for (int half = 0; half < 2; ++half) {
    const int j = half * 256 + wave * 64 + lane;    // staged column j <-> image column x0 - 128 + j
    const int x = x0 - 128 + j;
    const bool set = x >= 0 && x < W && masks[row + x] >= 0.5f;
    const unsigned long long b = __ballot(set);
    if (lane == 0) bits[j >> 6] = b;
  }
  __syncthreads();
  const int x = x0 + tid;
  if (x >= W) return;
  const int p = 128 + tid, b = p & 63;
  int d = 1 << 20;
  {  // to the left, the pixel itself included: at most three words cover 128 columns
    int wi = p >> 6;
    unsigned long long m = bits[wi] & (b == 63 ? ~0ull : ((1ull << (b + 1)) - 1ull));
    for (int k = 0; k < 3; ++k) {
      if (m) {
        d = p - (wi * 64 + 63 - __clzll((long long)m));
        break;
      }
      if (--wi < 0) break;
      m = bits[wi];
    }
  }
  {  // to the right
    int wi = p >> 6;
    unsigned long long m = bits[wi] & (~0ull << b);
    for (int k = 0; k < 3; ++k) {
      if (m) {
        d = min(d, wi * 64 + (__ffsll((unsigned long long)m) - 1) - p);
        break;
      }
      if (++wi > 7) break;
      m = bits[wi];
    }
  }
  dist[row + x] = d > TR_MAX_R ? TR_FAR : (unsigned char)d;
}

// out (M, H + 2, W + 2): the frame is 1; interior (y, x) is 1 iff some row y + dy, |dy| <= r, inside the image has a set
// pixel within half[dy + r] columns of x.  A block stages rows y0 - r ... y0 + 63 + r of its 64 columns of `dist` in LDS.
__global__ void __launch_bounds__(TR_THREADS) k_dilate(int H, int W, int r, HalfTable tbl, const unsigned char* __restrict__ dist,
                                                       unsigned char* __restrict__ out) {
  __shared__ unsigned char tile[(TR_TILE + 2 * TR_MAX_R) * TR_TILE];
  __shared__ unsigned char half[2 * TR_MAX_R + 2];
  const int tid = threadIdx.x, c = tid & 63, q = tid >> 6;
  const int X0 = blockIdx.x * TR_TILE, Y0 = blockIdx.y * TR_TILE;       // padded coordinates of the tile's corner
  const long long img = (long long)blockIdx.z * H * W;
  half[tid] = tbl.h[tid];
  const int x = X0 - 1 + c, rows = TR_TILE + 2 * r;
  for (int i = q; i < rows; i += TR_THREADS / 64) {
    const int y = Y0 - 1 - r + i;
    tile[i * TR_TILE + c] = (x >= 0 && x < W && y >= 0 && y < H) ? dist[img + (long long)y * W + x] : TR_FAR;
  }
  __syncthreads();
  const int X = X0 + c;
  if (X >= W + 2) return;
  unsigned char* o = out + (long long)blockIdx.z * (H + 2) * (W + 2);
  for (int j = 0; j < TR_TILE / 4; ++j) {
    const int ly = q * (TR_TILE / 4) + j, Y = Y0 + ly;
    if (Y >= H + 2) break;
    int hit = (X == 0 || X == W + 1 || Y == 0 || Y == H + 1) ? 1 : 0;
    if (!hit) {
      const unsigned char* col = tile + ly * TR_TILE + c;
      for (int k = 0; k <= 2 * r; ++k) hit |= col[k * TR_TILE] <= half[k] ? 1 : 0;
    }
    o[(long long)Y * (W + 2) + X] = (unsigned char)hit;
  }
}

// ---- vertex test -----------------------------------------------------------------------------------------------------------
// extract_by_mc.py:85-87, 98 in fp64 and in numpy's order of operations; cams (M, 21) = [K | R | t] row-major, read with
// wave-uniform indices (scalar loads: nothing writes the table during the launch).
__device__ __forceinline__ double tr_dot3(const double* __restrict__ a, double x, double y, double z) {
  return a[0] * x + a[1] * y + a[2] * z;           // left to right, no contraction (file-wide pragma)
}

// rint(u) + 1 clipped to [0, hi]; NaN and everything `astype(int32)` cannot hold end on the frame (0 or hi, both ones)
__device__ __forceinline__ int tr_pixel(double u, int hi) {
  double v = rint(u) + 1.0;
  if (!(v >= 0.0)) v = 0.0;
  if (v > (double)hi) v = (double)hi;
  return (int)v;
}

__global__ void __launch_bounds__(TR_THREADS) k_points_in_masks(long long N, const float* __restrict__ pts, int M, int H, int W,
                                                                const unsigned char* __restrict__ padded,
                                                                const double* __restrict__ cams, unsigned char* __restrict__ keep) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i >= N) return;
  const double px = (double)pts[i * 3], py = (double)pts[i * 3 + 1], pz = (double)pts[i * 3 + 2];
  const long long plane = (long long)(H + 2) * (W + 2);
  int inside = 1;
  for (int m = 0; m < M && inside; ++m) {
    const double* K = cams + (long long)m * 21;
    const double *R = K + 9, *t = K + 18;
    const double qx = tr_dot3(R, px, py, pz) + t[0], qy = tr_dot3(R + 3, px, py, pz) + t[1], qz = tr_dot3(R + 6, px, py, pz) + t[2];
    const double ux = tr_dot3(K, qx, qy, qz), uy = tr_dot3(K + 3, qx, qy, qz), uz = tr_dot3(K + 6, qx, qy, qz);
    const int ix = tr_pixel(ux / uz, W + 1), iy = tr_pixel(uy / uz, H + 1);
    inside = padded[m * plane + (long long)iy * (W + 2) + ix] != 0;
  }
  keep[i] = (unsigned char)inside;
}

// ---- stable compaction -----------------------------------------------------------------------------------------------------
// Three launches: per-block counts (k_flag_count), an exclusive scan of the block counts by one block (k_scan_totals, any
// number of blocks, 1024 at a time with a carry), and the emit pass, which recomputes the in-block prefix from the ballots.
struct VertexFlag {                                  // keep[i] != 0; emits new_index and optionally moves a row of floats
  const unsigned char* keep;
  int* new_index;
  const float* rows;
  float* out_rows;
  int width;
  __device__ __forceinline__ bool flag(long long i) const { return keep[i] != 0; }
  __device__ __forceinline__ void emit(long long i, bool s, int pos) const {
    new_index[i] = s ? pos : -1;
    if (s && rows)
      for (int k = 0; k < width; ++k) out_rows[(long long)pos * width + k] = rows[i * width + k];
  }
};

struct FaceFlag {                                    // all three vertices survive (and face_keep[f], if given)
  const int* faces;
  const unsigned char* face_keep;
  const int* new_index;
  long long N;
  int* out_faces;
  int* bad;                                          // set when a vertex index lies outside [0, N)
  __device__ __forceinline__ bool flag(long long f) const {
    if (face_keep && !face_keep[f]) return false;
    bool s = true;
    for (int k = 0; k < 3; ++k) {
      const int v = faces[f * 3 + k];
      if (v < 0 || v >= N) {
        atomicOr(bad, 1);
        return false;
      }
      s = s && new_index[v] >= 0;
    }
    return s;
  }
  __device__ __forceinline__ void emit(long long f, bool s, int pos) const {
    if (!s) return;
    for (int k = 0; k < 3; ++k) out_faces[(long long)pos * 3 + k] = new_index[faces[f * 3 + k]];
  }
};

template <class Flag>
__global__ void __launch_bounds__(TR_SCAN) k_flag_count(Flag fl, long long n, int* __restrict__ block_sums) {
  __shared__ int wsum[TR_SCAN / 64];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * TR_SCAN + tid;
  const unsigned long long b = __ballot(i < n && fl.flag(i));
  if ((tid & 63) == 0) wsum[tid >> 6] = __popcll(b);
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int w = 0; w < TR_SCAN / 64; ++w) s += wsum[w];
    block_sums[blockIdx.x] = s;
  }
}

// in place: sums[b] <- sum of sums[0 .. b - 1]; total[0] <- the sum of all
__global__ void __launch_bounds__(TR_SCAN) k_scan_totals(int* __restrict__ sums, int nb, int* __restrict__ total) {
  __shared__ int wsum[TR_SCAN / 64];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < nb; base += TR_SCAN) {
    const int v = base + tid < nb ? sums[base + tid] : 0;
    int inc = v;                                     // inclusive scan inside the wave
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o, 64);
      if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = carry_s;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (base + tid < nb) sums[base + tid] = before + inc - v;
    __syncthreads();
    if (tid == TR_SCAN - 1) carry_s = before + inc;
    __syncthreads();
  }
  if (tid == 0) total[0] = carry_s;
}

template <class Flag>
__global__ void __launch_bounds__(TR_SCAN) k_flag_emit(Flag fl, long long n, const int* __restrict__ block_offsets) {
  __shared__ int wsum[TR_SCAN / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long i = (long long)blockIdx.x * TR_SCAN + tid;
  const bool s = i < n && fl.flag(i);
  const unsigned long long b = __ballot(s);
  if (lane == 0) wsum[wave] = __popcll(b);
  __syncthreads();
  int pos = block_offsets[blockIdx.x] + __popcll(b & ((1ull << lane) - 1ull));
  for (int w = 0; w < wave; ++w) pos += wsum[w];
  if (i < n) fl.emit(i, s, pos);
}

template <class Flag>
static int compact(const Flag& fl, long long n, int* count, int* workspace, hipStream_t stream) {
  const long long blocks = (n + TR_SCAN - 1) / TR_SCAN;
  hipLaunchKernelGGL(k_flag_count<Flag>, dim3((unsigned)blocks), dim3(TR_SCAN), 0, stream, fl, n, workspace);
  hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(TR_SCAN), 0, stream, workspace, (int)blocks, count);
  hipLaunchKernelGGL(k_flag_emit<Flag>, dim3((unsigned)blocks), dim3(TR_SCAN), 0, stream, fl, n, (const int*)workspace);
  return ndjir_check_launch();
}

// ---- face components -------------------------------------------------------------------------------------------------------
// status bits
constexpr int CC_FULL = 1, CC_SPIN = 2, CC_INDEX = 4;
constexpr unsigned long long CC_EMPTY = ~0ull;
constexpr int CC_HOOK_TRIES = 1 << 16;

template <class T>
__device__ __forceinline__ T cc_load(const T* p) {    // what another workgroup may have written in this launch
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(TR_THREADS) k_cc_init(long long F, long long slots, unsigned long long* __restrict__ keys,
                                                        int* __restrict__ owner, int* __restrict__ parent, int* __restrict__ status) {
  const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (i < slots) {
    keys[i] = CC_EMPTY;
    owner[i] = -1;
  }
  if (i < F) parent[i] = (int)i;
  if (i == 0) status[0] = 0;
}

// Root of x with path halving.  parent[v] <= v always holds (a root is hooked under a smaller root only, halving moves a
// node to an ancestor), so every step strictly decreases x: at most x + 1 steps, whatever a stale read returns.
__device__ __forceinline__ int cc_find(int* parent, int x) {
  for (;;) {
    const int p = cc_load(parent + x);
    if (p == x) return x;
    const int g = cc_load(parent + p);
    if (g == p) return p;
    atomicMin(parent + x, g);
    x = g;
  }
}

__device__ __forceinline__ void cc_unite(int* parent, int a, int b, int* status) {
  for (int tries = 0; tries < CC_HOOK_TRIES; ++tries) {
    a = cc_find(parent, a);
    b = cc_find(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    if (atomicCAS(parent + a, a, b) == a) return;      // the larger root goes under the smaller
  }
  atomicOr(status, CC_SPIN);
}

__device__ __forceinline__ unsigned long long cc_mix(unsigned long long k) {        // murmur3's 64-bit finaliser
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// one thread per (face, edge): claim or find the edge's slot, then meet the slot's first face
__global__ void __launch_bounds__(TR_THREADS) k_cc_edges(long long F, long long N, const int* __restrict__ faces, long long slots,
                                                         unsigned long long* keys, int* owner, int* parent, int* status) {
  const long long t = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (t >= 3 * F) return;
  const int f = (int)(t / 3), e = (int)(t - 3LL * f);
  const int u = faces[3LL * f + e], v = faces[3LL * f + (e == 2 ? 0 : e + 1)];
  if (u < 0 || v < 0 || u >= N || v >= N) {
    atomicOr(status, CC_INDEX);
    return;
  }
  if (u == v) return;                                 // a repeated vertex spans no edge
  const unsigned long long key = ((unsigned long long)(unsigned)min(u, v) << 32) | (unsigned)max(u, v);
  const unsigned long long mask = (unsigned long long)slots - 1ull;
  unsigned long long s = cc_mix(key) & mask;
  long long probes = 0;
  for (; probes < slots; ++probes, s = (s + 1) & mask) {
    unsigned long long k = cc_load(keys + s);
    if (k == CC_EMPTY) k = atomicCAS(keys + s, CC_EMPTY, key);
    if (k == CC_EMPTY || k == key) break;
  }
  if (probes >= slots) {
    atomicOr(status, CC_FULL);
    return;
  }
  const int first = atomicCAS(owner + s, -1, f);
  if (first != -1 && first != f) cc_unite(parent, f, first, status);
}

__global__ void __launch_bounds__(TR_THREADS) k_cc_flatten(long long F, int* parent) {
  const long long f = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
  if (f >= F) return;
  int r = (int)f;
  for (long long step = 0; step <= F; ++step) {       // strictly decreasing, see cc_find
    const int p = cc_load(parent + r);
    if (p == r) break;
    r = p;
  }
  __hip_atomic_store(parent + f, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

static inline unsigned tr_blocks(long long n) { return (unsigned)((n + TR_THREADS - 1) / TR_THREADS); }

}  // namespace ndjir

extern "C" int ndjir_mask_dilate(int M, int H, int W, const float* masks, int r, const int* half_widths, unsigned char* row_dist,
                                 unsigned char* out, hipStream_t stream) {
  using namespace ndjir;
  if (M <= 0) return NDJIR_OK;
  if (H <= 0 || W <= 0 || M > 65535 || H > 65535 || (long long)H * W > 0x7fffffffLL || r < 0 || r > TR_MAX_R) return NDJIR_ERR_ARG;
  if (!masks || !half_widths || !row_dist || !out) return NDJIR_ERR_ARG;
  HalfTable tbl;
  for (int k = 0; k < (int)sizeof(tbl.h); ++k) tbl.h[k] = 0;
  for (int k = 0; k <= 2 * r; ++k) {
    if (half_widths[k] < 0 || half_widths[k] > TR_MAX_R) return NDJIR_ERR_ARG;
    tbl.h[k] = (unsigned char)half_widths[k];
  }
  hipLaunchKernelGGL(k_row_dist, dim3((unsigned)((W + TR_THREADS - 1) / TR_THREADS), (unsigned)H, (unsigned)M), dim3(TR_THREADS), 0,
                     stream, H, W, masks, row_dist);
  const unsigned gy = (unsigned)((H + 2 + TR_TILE - 1) / TR_TILE);
  hipLaunchKernelGGL(k_dilate, dim3((unsigned)((W + 2 + TR_TILE - 1) / TR_TILE), gy, (unsigned)M), dim3(TR_THREADS), 0, stream, H, W, r,
                     tbl, (const unsigned char*)row_dist, out);
  return ndjir_check_launch();
}

extern "C" int ndjir_points_in_masks(long long N, const float* points, int M, int H, int W, const unsigned char* padded_masks,
                                     const double* cams, unsigned char* keep, hipStream_t stream) {
  using namespace ndjir;
  if (N <= 0) return NDJIR_OK;
  if (M < 0 || H <= 0 || W <= 0 || N > 0x7fffffffLL || !points || !keep || (M > 0 && (!padded_masks || !cams))) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(k_points_in_masks, dim3(tr_blocks(N)), dim3(TR_THREADS), 0, stream, N, points, M, H, W, padded_masks, cams, keep);
  return ndjir_check_launch();
}

extern "C" int ndjir_compact_flags(long long N, const unsigned char* keep, int* new_index, int* count, int* workspace,
                                   const float* rows, int row_width, float* out_rows, hipStream_t stream) {
  using namespace ndjir;
  if (N < 0 || N > 0x7fffffffLL || !count) return NDJIR_ERR_ARG;
  if (hipMemsetAsync(count, 0, 2 * sizeof(int), stream) != hipSuccess) return NDJIR_ERR_LAUNCH;
  if (N == 0) return NDJIR_OK;
  if (!keep || !new_index || !workspace || (rows && (!out_rows || row_width <= 0))) return NDJIR_ERR_ARG;
  return compact(VertexFlag{keep, new_index, rows, out_rows, row_width}, N, count, workspace, stream);
}

extern "C" int ndjir_trim_faces(long long F, const int* faces, const unsigned char* face_keep, long long N, const int* new_index,
                                int* out_faces, int* count, int* workspace, hipStream_t stream) {
  using namespace ndjir;
  if (F < 0 || F > 0x7fffffffLL / 3 || N < 0 || N > 0x7fffffffLL || !count) return NDJIR_ERR_ARG;
  if (hipMemsetAsync(count, 0, 2 * sizeof(int), stream) != hipSuccess) return NDJIR_ERR_LAUNCH;
  if (F == 0) return NDJIR_OK;
  if (!faces || !out_faces || !workspace || (N > 0 && !new_index)) return NDJIR_ERR_ARG;
  return compact(FaceFlag{faces, face_keep, new_index, N, out_faces, count + 1}, F, count, workspace, stream);
}

extern "C" int ndjir_face_components(long long F, const int* faces, long long N, long long slots, unsigned long long* keys, int* owner,
                                     int* labels, int* status, hipStream_t stream) {
  using namespace ndjir;
  if (F < 0 || F > 0x7fffffffLL / 3 || N < 0 || N > 0x7fffffffLL) return NDJIR_ERR_ARG;
  if (F == 0) return NDJIR_OK;
  if (slots < 1 || slots > (1LL << 40) || (slots & (slots - 1)) || !faces || !keys || !owner || !labels || !status) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(k_cc_init, dim3(tr_blocks(slots > F ? slots : F)), dim3(TR_THREADS), 0, stream, F, slots, keys, owner, labels, status);
  hipLaunchKernelGGL(k_cc_edges, dim3(tr_blocks(3 * F)), dim3(TR_THREADS), 0, stream, F, N, faces, slots, keys, owner, labels, status);
  hipLaunchKernelGGL(k_cc_flatten, dim3(tr_blocks(F)), dim3(TR_THREADS), 0, stream, F, labels);
  if (ndjir_check_launch() != NDJIR_OK) return NDJIR_ERR_LAUNCH;
  int st = 0;                                         // the one place this file waits for the device: the error code
  if (hipMemcpyAsync(&st, status, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess) return NDJIR_ERR_LAUNCH;
  if (hipStreamSynchronize(stream) != hipSuccess) return NDJIR_ERR_LAUNCH;
  if (st & CC_FULL) return NDJIR_ERR_CAPACITY;
  return st ? NDJIR_ERR_ARG : NDJIR_OK;
}
