// Class-label images -> object maps (dm_orth_project_labels): orth_project of the one-hot value map
// value[b, c, y, x] = (label[b, 0, y, x] == c), without that value map.
//
// Native route (max / min, up to DM_LABEL_NATIVE_MAX_CLASSES classes): for max and min the result of a
// cell is decided by WHICH classes were seen in it, one bit per class.
//   k_label_sets    per pixel: the cell once, by project_pixel (the library's exact pixel arithmetic),
//                   then the pixel's class bit OR-ed into the cell's 64-bit word of a (B, mh, mw) plane
//                   in the workspace (bit c = class c seen, bit 63 = a label outside [0, C) seen;
//                   word != 0 = the cell was hit).  Lanes of a wave that share a cell combine first.
//   k_label_expand  per group of four cells: the words -> all C channels of out and mask.
// With v_max[c] = seen[c] ? 1 : 0 and v_min[c] = (another class or an out-of-range label seen) ? 0 : 1 a
// channel of a cell holds one of three values: the fill (not hit), reduce(fill, 0) or reduce(fill, 1),
// reduce being torch_scatter's "store only if new > old" (new < old for min), so that a NaN fill stays.
// The height map is the library's heights projection (dm_orth_project_f32, vc = 0, fill -inf, max).
//
// Compatibility route (sum / mean / prod, more classes, fill -0.0): k_labels_one_hot expands the labels
// to the float32 one-hot tensor in the workspace and dm_orth_project_f32 runs on it.
#include <stddef.h>
#include <string.h>

#include "dm_kernels.hpp"

namespace dm {
namespace {

thread_local int g_label_route = 0;     // dm_debug_last_label_route

constexpr int kLabelFramesPerLaunch = 32;     // camera states that travel in one launch's arguments
constexpr int kCamFloats = 24;                // Cam's 23 floats, padded
constexpr unsigned long long kOtherBit = 1ull << 63;

struct LabelSetArgs {
  View v;
  int valid_c, num_classes;
  int b0, pad;                               // first frame of this launch
  const float* depth;
  const void* labels;
  const uint8_t* valid;
  unsigned long long* sets;
  float cams[kLabelFramesPerLaunch][kCamFloats];
};
static_assert(sizeof(LabelSetArgs) <= 4096, "kernel arguments are limited to 4 KiB");

// One thread per pixel; grid = (ceil(H*W / 256), 1, frames of this launch).
template <class T>
__global__ void __launch_bounds__(256) k_label_sets(LabelSetArgs a) {
  const int bl = blockIdx.z, b = a.b0 + bl;
  const int N = a.v.H * a.v.W;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  // this frame's camera state: scalar loads from the kernel arguments
  typedef const __attribute__((address_space(4))) float cfloat;
  cfloat* const pc = (cfloat*)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() +
                               offsetof(LabelSetArgs, cams)) + bl * kCamFloats;
  Cam cam;
#pragma unroll
  for (int k = 0; k < 9; ++k) { cam.p[k] = pc[k]; cam.y[k] = pc[9 + k]; }
  cam.h = pc[18]; cam.tx = pc[19]; cam.tz = pc[20]; cam.wo = pc[21]; cam.ho = pc[22];
  int cell = -1;
  unsigned long long bits = 0;
  if (i < N) {
    const int r = i / a.v.W, q = i - r * a.v.W;
    bool ok = border_ok(a.v, r, q);
    if (a.valid) ok = ok && a.valid[(size_t)b * N + i] != 0;
    const float z = a.depth[(size_t)b * N + i];
    cell = project_pixel(a.v, cam, z, ray_x(a.v, q), ray_y(a.v, r), ok).cell;
    if (cell >= 0) {
      const long long l = (long long)static_cast<const T*>(a.labels)[(size_t)b * N + i];
      bits = (unsigned long long)l < (unsigned long long)a.num_classes ? 1ull << l : kOtherBit;
    }
  }
  // Neighbouring pixels mostly share a cell: every lane gathers the bits of the lanes behind it that hold
  // its cell (a lane only ever takes bits of its own cell), and the first lane of each run of equal
  // cells -- which then holds the whole run -- issues the one atomic.
  const int lane = threadIdx.x & 63;
  uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int oc = __shfl_down(cell, d, 64);
    const uint32_t olo = __shfl_down(lo, d, 64), ohi = __shfl_down(hi, d, 64);
    if (lane + d < 64 && oc == cell) { lo |= olo; hi |= ohi; }
  }
  const int before = __shfl_up(cell, 1, 64);
  if (cell >= 0 && (lane == 0 || before != cell)) {
    bits = (unsigned long long)lo | ((unsigned long long)hi << 32);
    unsigned long long* w = a.sets + (size_t)b * a.v.mh * a.v.mw + cell;
    // (no look at the word first to skip bits it already holds: the dependent load in front of the
    // atomic cost more than the atomics it saved -- cfg3, 599 -> 221 us per 32 frames)
    atomicOr(w, bits);
  }
}

// torch_scatter's update rule on the fill value: the new value is stored only where it compares
// greater (max) / smaller (min), so a NaN fill stays
template <bool IS_MAX>
__device__ inline float reduce_fill(float fill, float v) {
  return (IS_MAX ? v > fill : v < fill) ? v : fill;
}

struct CellValues {
  float f, z, o;          // not hit (fill), reduce(fill, 0), reduce(fill, 1)
  uint32_t mz, mo;        // their masks (the fill's is 0)
};
template <bool IS_MAX>
__device__ inline CellValues cell_values(float fill) {
  CellValues c;
  c.f = fill;
  c.z = reduce_fill<IS_MAX>(fill, 0.0f);
  c.o = reduce_fill<IS_MAX>(fill, 1.0f);
  c.mz = mask_of(c.z, fill);
  c.mo = mask_of(c.o, fill);
  return c;
}
// channel `bit` of a cell whose class word is `w`: max -> 1 where the class was seen; min -> 1 where
// nothing else was
template <bool IS_MAX>
__device__ inline bool is_one(unsigned long long w, unsigned long long bit) {
  return IS_MAX ? (w & bit) != 0 : (w & ~bit) == 0;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Four cells per thread, all channels: 16-byte map stores (NT: non-temporal, dm_pixel.hpp
// kFillCachePolicy's reasoning), 4-byte mask stores.  grid = (ceil(M/4 / 256), B); M % 4 == 0.
template <bool IS_MAX, bool NT>
__global__ void __launch_bounds__(256)
k_label_expand(const unsigned long long* __restrict__ sets, float* __restrict__ out,
               uint8_t* __restrict__ mask, int C, int M, float fill) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (M >> 2)) return;
  const size_t b = blockIdx.y;
  const ulonglong2* sp = reinterpret_cast<const ulonglong2*>(sets + b * M + ((size_t)g << 2));
  const ulonglong2 s01 = sp[0], s23 = sp[1];
  const unsigned long long w[4] = {s01.x, s01.y, s23.x, s23.y};
  const CellValues cv = cell_values<IS_MAX>(fill);
  float* o = out + b * C * M + ((size_t)g << 2);
  uint8_t* m = mask + b * C * M + ((size_t)g << 2);
  for (int c = 0; c < C; ++c, o += M, m += M) {
    const unsigned long long bit = 1ull << c;
    f32x4 val;
    uint32_t mk = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool hit = w[k] != 0, one = is_one<IS_MAX>(w[k], bit);
      val[k] = hit ? (one ? cv.o : cv.z) : cv.f;
      mk |= (hit ? (one ? cv.mo : cv.mz) : 0u) << (8 * k);
    }
    if (NT) __builtin_nontemporal_store(val, reinterpret_cast<f32x4*>(o));
    else *reinterpret_cast<f32x4*>(o) = val;
    *reinterpret_cast<uint32_t*>(m) = mk;
  }
}

// Cell by cell, for map sizes that are not a multiple of four cells (or misaligned maps).
// grid = (ceil(M / 256), B).
template <bool IS_MAX>
__global__ void __launch_bounds__(256)
k_label_expand_cells(const unsigned long long* __restrict__ sets, float* __restrict__ out,
                     uint8_t* __restrict__ mask, int C, int M, float fill) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const size_t b = blockIdx.y;
  const unsigned long long w = sets[b * M + i];
  const CellValues cv = cell_values<IS_MAX>(fill);
  float* o = out + b * C * M + i;
  uint8_t* m = mask + b * C * M + i;
  for (int c = 0; c < C; ++c, o += M, m += M) {
    const bool hit = w != 0, one = is_one<IS_MAX>(w, 1ull << c);
    *o = hit ? (one ? cv.o : cv.z) : cv.f;
    *m = (uint8_t)(hit ? (one ? cv.mo : cv.mz) : 0u);
  }
}

// labels (B, n) -> one-hot (B, C, n) float32; a label outside [0, C) is an all-zero row.
// grid = (ceil(n / 256), B).
template <class T>
__global__ void __launch_bounds__(256)
k_labels_one_hot(const T* __restrict__ labels, float* __restrict__ out, int C, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t b = blockIdx.y;
  const long long l = (long long)labels[b * n + i];
  float* o = out + b * C * n + i;
  for (int c = 0; c < C; ++c, o += n) *o = l == c ? 1.0f : 0.0f;
}

hipError_t run_one_hot(const void* labels, int dtype, int C, int B, int n, float* out, hipStream_t s) {
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)B);
  switch (dtype) {
    case DM_LABEL_U8: hipLaunchKernelGGL(k_labels_one_hot<uint8_t>, grid, dim3(256), 0, s, static_cast<const uint8_t*>(labels), out, C, n); break;
    case DM_LABEL_I16: hipLaunchKernelGGL(k_labels_one_hot<int16_t>, grid, dim3(256), 0, s, static_cast<const int16_t*>(labels), out, C, n); break;
    case DM_LABEL_I32: hipLaunchKernelGGL(k_labels_one_hot<int32_t>, grid, dim3(256), 0, s, static_cast<const int32_t*>(labels), out, C, n); break;
    default: hipLaunchKernelGGL(k_labels_one_hot<long long>, grid, dim3(256), 0, s, static_cast<const long long*>(labels), out, C, n); break;
  }
  return hipGetLastError();
}

bool known_dtype(int dtype) { return dtype >= DM_LABEL_U8 && dtype <= DM_LABEL_I64; }

// Which route a call takes: a pure function of the parameters (the workspace is sized by it).
bool native_route(const dm_params& p, int C) {
  uint32_t fill_bits;
  memcpy(&fill_bits, &p.fill, sizeof fill_bits);
  // (a fill of -0.0 against the value +0.0: the existing routes order the two zeros, the rule above
  // does not -- left to them)
  return (p.reduction == DM_REDUCE_MAX || p.reduction == DM_REDUCE_MIN) &&
         C <= DM_LABEL_NATIVE_MAX_CLASSES && fill_bits != 0x80000000u;
}

dm_params heights_params(const dm_params& p) {      // the height map of a value-map call (maps.py:332-350)
  dm_params q = p;
  q.vc = 0;
  q.fill = -__builtin_inff();
  q.reduction = DM_REDUCE_MAX;
  return q;
}
dm_params one_hot_params(const dm_params& p, int C) {
  dm_params q = p;
  q.vc = C;
  return q;
}

// the expansion's cache policy: dm_debug_force_nt_fill's setting, else non-temporal where the maps and
// masks are more than the Infinity Cache could keep (dm_strip.hip nt_fill_pays)
bool nt_expand(const dm_params& p, int C) {
  const int forced = dm_debug_force_nt_fill(-1);
  dm_debug_force_nt_fill(forced);
  if (forced >= 0) return forced != 0;
  return (size_t)p.B * C * p.mh * p.mw * 5 > ((size_t)128 << 20);
}

// Workspace of a call: the route's own regions, then the workspace of the dm_orth_project_f32 call (`inner`)
//   native:  class words (B, mh, mw) u64 | mask of the height map (B, mh, mw), not returned | heights projection
//   compat:  one-hot value map (B, C, H, W) f32 | value-map projection
struct LabelWs { unsigned long long* sets; uint8_t* height_mask; float* one_hot; dm_params inner; };
LabelWs label_layout(Arena& a, const dm_params& p, int C) {
  LabelWs w = {};
  if (native_route(p, C)) {
    const size_t cells = (size_t)p.B * p.mh * p.mw;
    w.sets = a.take<unsigned long long>(cells);
    w.height_mask = a.take<uint8_t>(cells);
    w.inner = heights_params(p);
  } else {
    w.one_hot = a.take<float>((size_t)p.B * C * p.H * p.W);
    w.inner = one_hot_params(p, C);
  }
  return w;
}

int check_label_call(const dm_params* p, int dtype, int C) {
  int rc = validate_params(p);
  if (rc != DM_OK) return rc;
  if (C < 1) return set_error(DM_ERR_INVALID_ARGUMENT, "num_classes=%d must be >= 1", C);
  if (p->dc != 1)
    return set_error(DM_ERR_INVALID_ARGUMENT, "a label map needs a one-channel depth map (dc=%d)", p->dc);
  if (p->vc != 0)
    return set_error(DM_ERR_INVALID_ARGUMENT, "vc=%d must be 0 on entry: the labels are the value map", p->vc);
  if (!known_dtype(dtype)) return set_error(DM_ERR_INVALID_ARGUMENT, "unknown label dtype code %d", dtype);
  if (C > 65535) return set_error(DM_ERR_UNSUPPORTED, "num_classes is limited to 65535 per call");
  if ((int64_t)C * p->H * p->W >= (1ll << 40) || (int64_t)C * p->mh * p->mw >= (1ll << 40))
    return set_error(DM_ERR_UNSUPPORTED, "num_classes times the image or map size is out of range");
  return DM_OK;
}

}  // namespace
}  // namespace dm

extern "C" {

int dm_debug_last_label_route(void) { return dm::g_label_route; }

size_t dm_orth_project_labels_workspace_bytes(const dm_params* p, int32_t label_dtype, int32_t num_classes) {
  using namespace dm;
  if (check_label_call(p, label_dtype, num_classes) != DM_OK) return 0;
  Arena a;
  const LabelWs w = label_layout(a, *p, num_classes);
  a.take<unsigned char>(dm_orth_project_workspace_bytes(&w.inner));
  return a.used();
}

int dm_labels_one_hot_f32(const void* labels_dev, int32_t label_dtype, int32_t num_classes, int64_t B,
                          size_t n, float* out_dev, void* stream) {
  using namespace dm;
  if (!known_dtype(label_dtype))
    return set_error(DM_ERR_INVALID_ARGUMENT, "unknown label dtype code %d", label_dtype);
  if (num_classes < 1 || num_classes > 65535 || B < 0 || B > 65535 || n >= ((size_t)1 << 31))
    return set_error(DM_ERR_INVALID_ARGUMENT, "bad shape B=%lld num_classes=%d n=%zu", (long long)B, num_classes, n);
  if (B == 0 || n == 0) return DM_OK;
  if (!labels_dev || !out_dev) return set_error(DM_ERR_INVALID_ARGUMENT, "labels/out must not be NULL");
  g_label_route = DM_LABEL_ROUTE_COMPAT;
  const hipError_t e = run_one_hot(labels_dev, label_dtype, num_classes, (int)B, (int)n, out_dev,
                                   static_cast<hipStream_t>(stream));
  return launch_status(e);
}

int dm_orth_project_labels(const dm_params* p, const dm_frame* frames, const float* depth_dev,
                           const void* labels_dev, int32_t label_dtype, int32_t num_classes,
                           const uint8_t* valid_dev, float* out_dev, uint8_t* mask_dev, float* height_dev,
                           void* workspace_dev, size_t workspace_bytes, int32_t* status_dev, void* stream) {
  using namespace dm;
  int rc = check_label_call(p, label_dtype, num_classes);
  if (rc != DM_OK) return rc;
  if (p->B == 0) return DM_OK;
  if (!frames || !depth_dev || !labels_dev || !out_dev || !mask_dev)
    return set_error(DM_ERR_INVALID_ARGUMENT, "frames/depth/labels/out/mask must not be NULL");
  if ((p->valid_c > 0) != (valid_dev != nullptr))
    return set_error(DM_ERR_INVALID_ARGUMENT, "valid pointer and valid_c=%d disagree", p->valid_c);
  rc = check_workspace(workspace_dev, workspace_bytes,
                       dm_orth_project_labels_workspace_bytes(p, label_dtype, num_classes));
  if (rc != DM_OK) return rc;
  Arena arena(workspace_dev, workspace_bytes);
  if (!arena.aligned()) return set_error(DM_ERR_INVALID_ARGUMENT, "the workspace must be 256-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int C = num_classes, N = p->H * p->W, M = p->mh * p->mw;
  const LabelWs w = label_layout(arena, *p, C);
  void* const inner_ws = arena.take<unsigned char>(0);      // (the rest: the projection's own workspace)

  if (!native_route(*p, C)) {
    g_label_route = DM_LABEL_ROUTE_COMPAT;
    rc = launch_status(run_one_hot(labels_dev, label_dtype, C, p->B, N, w.one_hot, s));
    if (rc != DM_OK) return rc;
    return dm_orth_project_f32(&w.inner, frames, depth_dev, w.one_hot, valid_dev, out_dev, mask_dev, height_dev,
                               nullptr, nullptr, inner_ws, arena.rest(), status_dev, stream);
  }

  g_label_route = DM_LABEL_ROUTE_NATIVE;
  unsigned long long* sets = w.sets;
  hipError_t e = hipMemsetAsync(sets, 0, (size_t)p->B * M * sizeof(*sets), s);
  LabelSetArgs a;
  a.v = make_view(*p);
  a.valid_c = p->valid_c;
  a.num_classes = C;
  a.pad = 0;
  a.depth = depth_dev;
  a.labels = labels_dev;
  a.valid = valid_dev;
  a.sets = sets;
  for (int b0 = 0; b0 < p->B && e == hipSuccess; b0 += kLabelFramesPerLaunch) {
    const int nb = p->B - b0 < kLabelFramesPerLaunch ? p->B - b0 : kLabelFramesPerLaunch;
    a.b0 = b0;
    for (int k = 0; k < nb; ++k) {
      const dm_frame& f = frames[b0 + k];
      float* c = a.cams[k];
      memcpy(c, f.Rp, 9 * sizeof(float));
      memcpy(c + 9, f.Ry, 9 * sizeof(float));
      c[18] = f.cam_height; c[19] = f.tx; c[20] = f.tz; c[21] = f.width_offset; c[22] = f.height_offset;
      c[23] = 0.0f;
    }
    const dim3 grid((unsigned)((N + 255) / 256), 1, (unsigned)nb);
    switch (label_dtype) {
      case DM_LABEL_U8: hipLaunchKernelGGL(k_label_sets<uint8_t>, grid, dim3(256), 0, s, a); break;
      case DM_LABEL_I16: hipLaunchKernelGGL(k_label_sets<int16_t>, grid, dim3(256), 0, s, a); break;
      case DM_LABEL_I32: hipLaunchKernelGGL(k_label_sets<int32_t>, grid, dim3(256), 0, s, a); break;
      default: hipLaunchKernelGGL(k_label_sets<long long>, grid, dim3(256), 0, s, a); break;
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    const bool is_max = p->reduction == DM_REDUCE_MAX;
    const bool vec = M % 4 == 0 && reinterpret_cast<uintptr_t>(out_dev) % 16 == 0 &&
                     reinterpret_cast<uintptr_t>(mask_dev) % 4 == 0;
    if (vec) {
      const dim3 grid((unsigned)((M / 4 + 255) / 256), (unsigned)p->B);
      const bool nt = nt_expand(*p, C);
#define DM_EXPAND(MAX, NT) hipLaunchKernelGGL((k_label_expand<MAX, NT>), grid, dim3(256), 0, s, sets, out_dev, mask_dev, C, M, p->fill)
      if (is_max) { if (nt) DM_EXPAND(true, true); else DM_EXPAND(true, false); }
      else { if (nt) DM_EXPAND(false, true); else DM_EXPAND(false, false); }
#undef DM_EXPAND
    } else {
      const dim3 grid((unsigned)((M + 255) / 256), (unsigned)p->B);
      if (is_max) hipLaunchKernelGGL(k_label_expand_cells<true>, grid, dim3(256), 0, s, sets, out_dev, mask_dev, C, M, p->fill);
      else hipLaunchKernelGGL(k_label_expand_cells<false>, grid, dim3(256), 0, s, sets, out_dev, mask_dev, C, M, p->fill);
    }
    e = hipGetLastError();
  }
  if (e != hipSuccess || !height_dev) return launch_status(e);
  return dm_orth_project_f32(&w.inner, frames, depth_dev, nullptr, valid_dev, height_dev, w.height_mask, nullptr,
                             nullptr, nullptr, inner_ws, arena.rest(), status_dev, stream);
}

}  // extern "C"
