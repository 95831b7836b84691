// Backward of orth_project (dm_orth_project_winners_f32 / dm_orth_project_backward_f32).
//
// Two passes over the pixels, both recomputing every pixel's cell and height with
// project_pixel -- the device code the forward's cells are tested bit-identical against -- so
// the backward sees exactly the cells the forward reduced into:
//  * winners: for max / min the lowest flat pixel index h*W+w whose value equals the cell's
//    result while the cell's changed-mask is set (torch_scatter's CPU argmax: a strict `>` in
//    index order); for mean the number of contributors of every cell.  Only CANDIDATES -- pixels
//    whose value equals the result -- issue an atomicMin, usually about one per cell (one-hot
//    value maps tie more).
//  * backward: per pixel the weight of its cell (winner: 1 / 0, sum: 1, mean: 1 / count) times
//    the incoming gradient, written to grad_value / grad_depth, plus four per-frame moments of
//    the height gradient w (sum w, w*X, w*Y, w*z) accumulated per thread over a grid-stride loop,
//    reduced through the wave and LDS, one float64 atomic add per moment per workgroup.  The host chains the moments through the
//    pitch rotation's derivative; the kernel stays free of it.
#include "dm_kernels.hpp"

namespace dm {

namespace {

// The channel of the output map / of the depth map a (frame, depth channel, value channel k)
// belongs to is the plain index arithmetic of the forward (k_scatter_generic).
template <int RED, bool HAS_WIN, bool HAS_HWIN>
__global__ void __launch_bounds__(256)
k_winners(View v, int dc, int vc, int valid_c, float fill, const dm_frame* __restrict__ frames,
          const float* __restrict__ depth, const float* __restrict__ value,
          const uint8_t* __restrict__ valid, const float* __restrict__ out,
          const float* __restrict__ height, unsigned* __restrict__ win,
          unsigned* __restrict__ hwin) {
  const int b = blockIdx.z, ch = blockIdx.y;
  const int N = v.H * v.W;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const Cam cam = load_cam(frames + b);
  const int r = i / v.W, q = i - r * v.W;
  bool ok = border_ok(v, r, q);
  if (valid) ok = ok && valid[((size_t)b * valid_c + (valid_c == 1 ? 0 : ch)) * N + i] != 0;
  const float z = depth[((size_t)b * dc + ch) * N + i];
  const Hit h = project_pixel(v, cam, z, ray_x(v, q), ray_y(v, r), ok);
  if (h.cell < 0) return;
  const size_t M = (size_t)v.mh * v.mw;
  if (HAS_WIN) {
    if (RED == DM_REDUCE_MEAN) {
      atomicAdd(win + ((size_t)b * dc + ch) * M + h.cell, 1u);     // counts per depth channel
    } else {
      const int k0 = vc ? (dc == 1 ? 0 : ch) : ch;
      const int k1 = vc ? (dc == 1 ? vc : ch + 1) : ch + 1;
      const int oc = vc ? vc : dc;
      for (int k = k0; k < k1; ++k) {
        const size_t idx = ((size_t)b * oc + k) * M + h.cell;
        const float val = vc ? value[((size_t)b * vc + k) * N + i] : h.y;
        const float res = out[idx];
        if (val == res && mask_of(res, fill)) atomicMin(win + idx, (unsigned)i);
      }
    }
  }
  if (HAS_HWIN) {
    const size_t idx = ((size_t)b * dc + ch) * M + h.cell;
    const float res = height[idx];
    if (h.y == res && mask_of(res, -__builtin_inff())) atomicMin(hwin + idx, (unsigned)i);
  }
}

__device__ inline double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  return x;
}

// Grid-stride over the pixels of one (frame, depth channel); grid = (gx, dc, B) with gx capped
// (backward_blocks): every workgroup's moments go to the same four addresses of its frame, so
// fewer, fuller workgroups keep those same-address atomics few.
template <int RED>
__device__ inline float pixel_backward(const View& v, const Cam& cam, int b, int ch, int i, int N, int dc,
                                       int vc, int valid_c, const uint8_t* __restrict__ valid,
                                       const float* __restrict__ depth, const unsigned* __restrict__ win,
                                       const unsigned* __restrict__ hwin, const float* __restrict__ gout,
                                       const float* __restrict__ gh, float* __restrict__ gval,
                                       float* __restrict__ gdep, float& X, float& Y, float& z) {
  const int r = i / v.W, q = i - r * v.W;
  bool ok = border_ok(v, r, q);
  if (valid) ok = ok && valid[((size_t)b * valid_c + (valid_c == 1 ? 0 : ch)) * N + i] != 0;
  z = depth[((size_t)b * dc + ch) * N + i];
  const float ax = ray_x(v, q), ay = ray_y(v, r);
  const Hit h = project_pixel(v, cam, z, ax, ay, ok);
  const size_t M = (size_t)v.mh * v.mw;
  const size_t dcell = ((size_t)b * dc + ch) * M + h.cell;     // (used only when h.cell >= 0)
  // weight of the pixel in its cell of output channel k (that cell's index idx) times the cell's gradient
  auto take = [&](size_t idx) -> float {
    if (RED == DM_REDUCE_MAX || RED == DM_REDUCE_MIN) return win[idx] == (unsigned)i ? gout[idx] : 0.0f;
    if (RED == DM_REDUCE_MEAN) return gout[idx] / (float)win[dcell];
    return gout[idx];
  };
  float w = 0.0f;
  if (vc) {
    if (gval) {
      const int k0 = dc == 1 ? 0 : ch, k1 = dc == 1 ? vc : ch + 1;
      for (int k = k0; k < k1; ++k) {
        const size_t idx = ((size_t)b * vc + k) * M + h.cell;
        gval[((size_t)b * vc + k) * N + i] = (h.cell >= 0 && gout) ? take(idx) : 0.0f;
      }
    }
    if (h.cell >= 0 && gh && hwin[dcell] == (unsigned)i) w = gh[dcell];
  } else if (h.cell >= 0 && gout) {
    w = take(dcell);
  }
  if (gdep) {
    // d y2 / d z: row 1 of the output rotation applied to d(x1, y1, z1)/dz = Rp^T (ax, ay, 1)
    const float d0 = ax * cam.p[0] + ay * cam.p[3] + cam.p[6];
    const float d1 = ax * cam.p[1] + ay * cam.p[4] + cam.p[7];
    const float d2 = ax * cam.p[2] + ay * cam.p[5] + cam.p[8];
    const float dy = v.to_global ? cam.y[1] * d0 + cam.y[4] * d1 + cam.y[7] * d2 : d1;
    gdep[((size_t)b * dc + ch) * N + i] = w * dy;
  }
  X = ax * z;
  Y = ay * z;
  return w;
}

template <int RED>
__global__ void __launch_bounds__(256)
k_backward(View v, int dc, int vc, int valid_c, const dm_frame* __restrict__ frames,
           const float* __restrict__ depth, const uint8_t* __restrict__ valid,
           const unsigned* __restrict__ win, const unsigned* __restrict__ hwin,
           const float* __restrict__ gout, const float* __restrict__ gh,
           float* __restrict__ gval, float* __restrict__ gdep, double* __restrict__ moments) {
  __shared__ double part[4][4];
  const int b = blockIdx.z, ch = blockIdx.y;
  const int N = v.H * v.W;
  const Cam cam = load_cam(frames + b);
  double m[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
    float X, Y, z;
    const float w = pixel_backward<RED>(v, cam, b, ch, i, N, dc, vc, valid_c, valid, depth, win, hwin, gout,
                                        gh, gval, gdep, X, Y, z);
    if (w != 0.0f) {
      m[0] += (double)w; m[1] += (double)w * X; m[2] += (double)w * Y; m[3] += (double)w * z;
    }
  }
  if (!moments) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < 4; ++j) m[j] = wave_sum(m[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) part[wave][j] = m[j];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const double s = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (s != 0.0) atomicAdd(moments + (size_t)b * 4 + threadIdx.x, s);
  }
}

// Workgroups per (frame, depth channel): enough for ~2048 in all (8 per CU), never more than the pixels need.
inline unsigned backward_blocks(const dm_params& p) {
  const long long need = ((long long)p.H * p.W + 255) / 256;
  long long want = 2048 / ((long long)p.B * p.dc);
  if (want < 16) want = 16;
  return (unsigned)(need < want ? need : want);
}

}  // namespace

hipError_t run_winners(const dm_params& p, const dm_frame* frames_host, const float* depth,
                       const float* value, const uint8_t* valid, const float* out,
                       const float* height, int32_t* win, int32_t* hwin, void* ws, hipStream_t s) {
  const size_t M = (size_t)p.mh * p.mw;
  const size_t oc = p.vc ? p.vc : p.dc;
  const bool mean = p.reduction == DM_REDUCE_MEAN;
  hipError_t e = hipMemcpyAsync(ws, frames_host, (size_t)p.B * sizeof(dm_frame), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return e;
  if (win) {
    e = hipMemsetAsync(win, mean ? 0 : 0xFF, (size_t)p.B * (mean ? p.dc : oc) * M * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
  }
  if (hwin) {
    e = hipMemsetAsync(hwin, 0xFF, (size_t)p.B * p.dc * M * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
  }
  const View v = make_view(p);
  const dm_frame* frames = static_cast<const dm_frame*>(ws);
  const dim3 grid((p.H * p.W + 255) / 256, p.dc, p.B);
  unsigned* w = reinterpret_cast<unsigned*>(win);
  unsigned* hw = reinterpret_cast<unsigned*>(hwin);
#define DM_LAUNCH(R, A, C)                                                                            \
  hipLaunchKernelGGL((k_winners<R, A, C>), grid, dim3(256), 0, s, v, p.dc, p.vc, p.valid_c, p.fill, \
                     frames, depth, value, valid, out, height, w, hw)
#define DM_CASE(R)                                        \
  case R:                                                 \
    if (w && hw) DM_LAUNCH(R, true, true);                \
    else if (w) DM_LAUNCH(R, true, false);                \
    else if (hw) DM_LAUNCH(R, false, true);               \
    break;
  switch (p.reduction) {
    DM_CASE(DM_REDUCE_MAX)
    DM_CASE(DM_REDUCE_MIN)
    DM_CASE(DM_REDUCE_SUM)
    DM_CASE(DM_REDUCE_MEAN)
    default: return hipErrorInvalidValue;
  }
#undef DM_CASE
#undef DM_LAUNCH
  return hipGetLastError();
}

hipError_t run_backward(const dm_params& p, const dm_frame* frames_host, const float* depth,
                        const uint8_t* valid, const int32_t* win, const int32_t* hwin,
                        const float* grad_out, const float* grad_height, float* grad_value,
                        float* grad_depth, double* moments, void* ws, hipStream_t s) {
  hipError_t e = hipMemcpyAsync(ws, frames_host, (size_t)p.B * sizeof(dm_frame), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) return e;
  if (moments) {
    e = hipMemsetAsync(moments, 0, (size_t)p.B * 4 * sizeof(double), s);
    if (e != hipSuccess) return e;
  }
  const View v = make_view(p);
  const dm_frame* frames = static_cast<const dm_frame*>(ws);
  const dim3 grid(backward_blocks(p), p.dc, p.B);
  const unsigned* w = reinterpret_cast<const unsigned*>(win);
  const unsigned* hw = reinterpret_cast<const unsigned*>(hwin);
#define DM_CASE(R)                                                                                  \
  case R:                                                                                           \
    hipLaunchKernelGGL((k_backward<R>), grid, dim3(256), 0, s, v, p.dc, p.vc, p.valid_c, frames,    \
                       depth, valid, w, hw, grad_out, grad_height, grad_value, grad_depth, moments); \
    break;
  switch (p.reduction) {
    DM_CASE(DM_REDUCE_MAX)
    DM_CASE(DM_REDUCE_MIN)
    DM_CASE(DM_REDUCE_SUM)
    DM_CASE(DM_REDUCE_MEAN)
    default: return hipErrorInvalidValue;
  }
#undef DM_CASE
  return hipGetLastError();
}

}  // namespace dm
