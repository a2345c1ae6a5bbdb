// bake.hip -- vertex textures of an extracted mesh and the environment map (export half).
//
// Reference: python/extract_by_mc.py:144-261.  `save_attributed_mesh` (:197-223) evaluates the geometric net, `nn.grad` and ONE
// material net per texture, six times per vertex, in host-fed batches; `create_rgb_color` (:187-194) places the net's output in an
// RGB triple; `extract_environment_map` (:226-261) evaluates the environment light net on an H x 2H lattice of directions built in
// numpy and quantises it on the host.  Here the four material nets run once on the packed sample input
// (network.material_nets_raw) and the kernels below turn their raw outputs into the six textures (k_bake_head, k_bake_scale),
// build the lattice (k_envmap_directions) and quantise the intensities (k_envmap_quantize).  One lane per vertex / pixel.
#include <hip/hip_runtime.h>

#include "common.h"

#pragma clang fp contract(off)

namespace ndjir {

constexpr int BK_THREADS = 256;

__device__ __forceinline__ float bk_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float bk_softplus(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // torch: beta 1, threshold 20
// np.clip(v, 0, 1) (:191-193): a NaN stays a NaN
__device__ __forceinline__ float bk_clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// `act_last` of the implicit-illumination net (python/network.py:331-334): 1 softplus(beta), 2 sigmoid, 3 relu
__device__ __forceinline__ float bk_last_act(int kind, float beta, float v) {
  if (kind == 1) {
    const float bv = beta * v;
    return bv > 20.f ? v : log1pf(expf(bv)) / beta;
  }
  if (kind == 2) return bk_sigmoid(v);
  return fmaxf(v, 0.f);
}

struct BakeCfg {
  int ci, cs;                // channels of the implicit-illumination / specular-reflectance nets (1 | 3)
  int act_imp;
  float beta_imp;
  int remap;                 // filament and remap: roughness^2, 0.16 s^2
  float lower_bound, spec_scale;
};

struct BakeOut {
  float *base_color, *implicit, *roughness, *specular, *roughness_std, *specular_std;
};

// Values in [0, 1] order like their bit patterns read as int, and a NaN's pattern lies above all of them: the integer
// maximum is the numpy maximum (NaN if any), whatever the order of the atomics.
__device__ __forceinline__ void bk_block_max(float v, int* dst) {
  __shared__ int part[BK_THREADS];
  part[threadIdx.x] = v != v ? 0x7fc00000 : __float_as_int(v);
  __syncthreads();
  for (int s = BK_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) part[threadIdx.x] = max(part[threadIdx.x], part[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicMax(dst, part[0]);
  __syncthreads();
}

__global__ void __launch_bounds__(BK_THREADS) k_bake_head(long long N, BakeCfg c, const float* __restrict__ raw_imp,
                                                          const float* __restrict__ raw_bc, const float* __restrict__ raw_r,
                                                          const float* __restrict__ raw_s, BakeOut o, int* __restrict__ std_max) {
  const long long p = (long long)blockIdx.x * BK_THREADS + threadIdx.x;
  float mr = 0.f, ms = 0.f;              // this lane's share of the two std maxima (0: the identity over [0, 1])
  if (p < N) {
    // base colour (python/network.py:262), fill_index -1
    for (int k = 0; k < 3; ++k) o.base_color[p * 3 + k] = bk_clip01(bk_sigmoid(raw_bc[p * 3 + k]));
    // implicit illumination (:331-334): blue when one channel (extract_by_mc.py:200-201)
    if (c.ci == 1) {
      o.implicit[p * 3] = 0.f;
      o.implicit[p * 3 + 1] = 0.f;
      o.implicit[p * 3 + 2] = bk_clip01(bk_last_act(c.act_imp, c.beta_imp, raw_imp[p]));
    } else {
      for (int k = 0; k < 3; ++k) o.implicit[p * 3 + k] = bk_clip01(bk_last_act(c.act_imp, c.beta_imp, raw_imp[p * 3 + k]));
    }
    // roughness (:456-463) and its std, green (extract_by_mc.py:202, 205)
    float r = bk_sigmoid(raw_r[p * 2]);
    if (c.remap) r = r * r;
    r = r < c.lower_bound ? c.lower_bound : (r > 1.f ? 1.f : r);
    const float rs = bk_clip01(bk_softplus(raw_r[p * 2 + 1]));
    o.roughness[p * 3] = 0.f;
    o.roughness[p * 3 + 1] = bk_clip01(r);
    o.roughness[p * 3 + 2] = 0.f;
    o.roughness_std[p * 3] = 0.f;
    o.roughness_std[p * 3 + 1] = rs;
    o.roughness_std[p * 3 + 2] = 0.f;
    mr = rs;
    // specular reflectance (:498-508) and its std: red when one channel (extract_by_mc.py:203-207)
    for (int k = 0; k < 3; ++k) {
      float v = 0.f, sd = 0.f;
      if (k < c.cs) {
        const float s = bk_sigmoid(raw_s[p * 2 * c.cs + k]);
        v = bk_clip01(c.remap ? 0.16f * (s * s) : c.spec_scale * s);
        sd = bk_clip01(bk_softplus(raw_s[p * 2 * c.cs + c.cs + k]));
        ms = (sd > ms || sd != sd) ? sd : ms;
      }
      o.specular[p * 3 + k] = v;
      o.specular_std[p * 3 + k] = sd;
    }
  }
  bk_block_max(mr, std_max);
  bk_block_max(ms, std_max + 1);
}

// `vertex_colors / vertex_colors.max()` of the two std textures (extract_by_mc.py:215-216): one correctly rounded division
__global__ void __launch_bounds__(BK_THREADS) k_bake_scale(long long n, float* __restrict__ roughness_std,
                                                           float* __restrict__ specular_std, const int* __restrict__ std_max) {
  const long long t = (long long)blockIdx.x * BK_THREADS + threadIdx.x;
  if (t >= n) return;
  roughness_std[t] = roughness_std[t] / __int_as_float(std_max[0]);
  specular_std[t] = specular_std[t] / __int_as_float(std_max[1]);
}

// np.linspace(a, b, n)[i] in double (numpy: i * step + a with step = (b - a) / (n - 1), the last element set to b)
__device__ __forceinline__ double bk_linspace(double a, double b, int n, int i) {
  if (i == n - 1) return b;
  const double step = (b - a) / (double)(n - 1);
  return (double)i * step + a;
}

__global__ void __launch_bounds__(BK_THREADS) k_envmap_directions(int H, float* __restrict__ dirs) {
  const int W = 2 * H;
  const long long t = (long long)blockIdx.x * BK_THREADS + threadIdx.x;
  if (t >= (long long)H * W) return;
  const int i = (int)(t / W), j = (int)(t - (long long)i * W);
  const double pi = 3.141592653589793;        // np.pi
  // extract_by_mc.py:229-235 (its `the` holds the column angle, its `phi` the row angle)
  const double row = bk_linspace(0.0, pi, H, i), col = bk_linspace(-pi, pi, W, j);
  const double sc = sin(col);
  dirs[t * 3] = (float)(cos(row) * sc);
  dirs[t * 3 + 1] = (float)(sin(row) * sc);
  dirs[t * 3 + 2] = (float)cos(col);
}

__global__ void __launch_bounds__(BK_THREADS) k_envmap_quantize(int H, int W, int C, const float* __restrict__ x,
                                                                const float* __restrict__ min_max, int sigmoid_mode,
                                                                unsigned char* __restrict__ image) {
  const long long t = (long long)blockIdx.x * BK_THREADS + threadIdx.x;
  if (t >= (long long)H * W) return;
  const float m = min_max[0], M = min_max[1];
  const int i = (int)(t / W), j = (int)(t - (long long)i * W);
  for (int k = 0; k < C; ++k) {
    float v = x[t * C + k];
    if (sigmoid_mode) v = v * 255.0f;
    else if (m != M) v = v / M * 255.0f;       // two correctly rounded fp32 operations, as in numpy (:247)
    else v = 255.0f;
    v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
    const unsigned char q = (unsigned char)(int)v;      // astype(np.uint8) of a value in [0, 255]: truncation
    // `[..., ::-1]` (:255): for three channels the writer (BGR) undoes it, for one it mirrors the row
    if (C == 1) image[(long long)i * W + (W - 1 - j)] = q;
    else image[t * 3 + k] = q;
  }
}

}  // namespace ndjir

extern "C" int ndjir_bake_head(long long N, const float* raw_implicit, const float* raw_base_color, const float* raw_roughness,
                               const float* raw_specular, int implicit_channels, int specular_channels, int implicit_act,
                               float implicit_beta, int remap, float roughness_lower_bound, float specular_scale,
                               float* const* textures, int* std_max, hipStream_t stream) {
  if (N <= 0) return NDJIR_OK;
  if (!raw_implicit || !raw_base_color || !raw_roughness || !raw_specular || !textures || !std_max) return NDJIR_ERR_ARG;
  for (int k = 0; k < 6; ++k)
    if (!textures[k]) return NDJIR_ERR_ARG;
  if ((implicit_channels != 1 && implicit_channels != 3) || (specular_channels != 1 && specular_channels != 3))
    return NDJIR_ERR_UNSUPPORTED;
  if (implicit_act < 1 || implicit_act > 3) return NDJIR_ERR_UNSUPPORTED;
  if (implicit_act == 1 && !(implicit_beta > 0.f)) return NDJIR_ERR_ARG;
  const long long blocks = (N + ndjir::BK_THREADS - 1) / ndjir::BK_THREADS;
  if (blocks > 0x7fffffffLL) return NDJIR_ERR_ARG;
  ndjir::BakeCfg c{implicit_channels, specular_channels, implicit_act, implicit_beta, remap, roughness_lower_bound, specular_scale};
  ndjir::BakeOut o{textures[0], textures[1], textures[2], textures[3], textures[4], textures[5]};
  hipLaunchKernelGGL(ndjir::k_bake_head, dim3((unsigned)blocks), dim3(ndjir::BK_THREADS), 0, stream, N, c, raw_implicit,
                     raw_base_color, raw_roughness, raw_specular, o, std_max);
  return ndjir::ndjir_check_launch();
}

extern "C" int ndjir_bake_scale(long long N, float* roughness_std, float* specular_std, const int* std_max, hipStream_t stream) {
  if (N <= 0) return NDJIR_OK;
  if (!roughness_std || !specular_std || !std_max) return NDJIR_ERR_ARG;
  const long long n = N * 3, blocks = (n + ndjir::BK_THREADS - 1) / ndjir::BK_THREADS;
  if (blocks > 0x7fffffffLL) return NDJIR_ERR_ARG;
  hipLaunchKernelGGL(ndjir::k_bake_scale, dim3((unsigned)blocks), dim3(ndjir::BK_THREADS), 0, stream, n, roughness_std,
                     specular_std, std_max);
  return ndjir::ndjir_check_launch();
}

extern "C" int ndjir_envmap_directions(int H, float* dirs, hipStream_t stream) {
  if (H < 2 || H > 16384 || !dirs) return NDJIR_ERR_ARG;
  const long long n = 2LL * H * H;
  hipLaunchKernelGGL(ndjir::k_envmap_directions, dim3((unsigned)((n + ndjir::BK_THREADS - 1) / ndjir::BK_THREADS)),
                     dim3(ndjir::BK_THREADS), 0, stream, H, dirs);
  return ndjir::ndjir_check_launch();
}

extern "C" int ndjir_envmap_quantize(int H, int W, int C, const float* intensity, const float* min_max, int sigmoid_mode,
                                     unsigned char* image, hipStream_t stream) {
  if (H <= 0 || W <= 0 || H > 16384 || W > 32768 || !intensity || !min_max || !image) return NDJIR_ERR_ARG;
  if (C != 1 && C != 3) return NDJIR_ERR_UNSUPPORTED;
  const long long n = (long long)H * W;
  hipLaunchKernelGGL(ndjir::k_envmap_quantize, dim3((unsigned)((n + ndjir::BK_THREADS - 1) / ndjir::BK_THREADS)),
                     dim3(ndjir::BK_THREADS), 0, stream, H, W, C, intensity, min_max, sigmoid_mode, image);
  return ndjir::ndjir_check_launch();
}
