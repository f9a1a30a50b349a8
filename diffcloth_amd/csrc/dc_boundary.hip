// Kernels of the whole-sweep device-pointer boundary (dc_*_schedule_dev, dc_get_states_dev, dc_get_force_schedule_gradients_dev ...):
// the caller's tensors — [slots][B][n][3], fp32 or fp64, xyz interleaved, the caller's vertex numbering — to and from the tape's planar
// fp32 [slots][B][3][n], every slot of an array in ONE launch; the cast of the small per-rollout data; the force-schedule gradients
// reduced on the device from the kept y tape. All of them are memory-bound: a lane moves 4 vertices (16 bytes per plane access) where
// n is a multiple of 4 and the pointers are 16-byte aligned, one vertex otherwise. Indices are `long` throughout.
#include <cstdint>
#include "dc_device.h"
#include "dc_primoffset.h"

namespace dc {
namespace {

constexpr int kThreads = 256;

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned blocks_for(long total) { return (unsigned) ((total + kThreads - 1) / kThreads); }

// 4 consecutive device vertices i .. i + 3 (i a multiple of 4) of one [n][3] block of the caller: a[3 j + d]. With a renumbering the caller's
// vertices are scattered (one 3-element access each); without one they are 12 consecutive elements, moved as 16-byte pieces when `wide`.
template <class T>
__device__ inline void load_xyz4(const T *__restrict__ blk, int i, const int *__restrict__ user_of, bool wide, float (&a)[12]) {
  if (user_of) {
    const int4 u = *reinterpret_cast<const int4 *>(user_of + i);
    const int uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const T *s = blk + 3 * (long) uu[j];
      a[3 * j] = (float) s[0]; a[3 * j + 1] = (float) s[1]; a[3 * j + 2] = (float) s[2];
    }
  } else if (wide) {
    if constexpr (sizeof(T) == 4) {
      const float4 *s = reinterpret_cast<const float4 *>(blk + 3 * (long) i);
      const float4 q0 = s[0], q1 = s[1], q2 = s[2];
      a[0] = q0.x; a[1] = q0.y; a[2] = q0.z; a[3] = q0.w; a[4] = q1.x; a[5] = q1.y; a[6] = q1.z; a[7] = q1.w;
      a[8] = q2.x; a[9] = q2.y; a[10] = q2.z; a[11] = q2.w;
    } else {
      const double2 *s = reinterpret_cast<const double2 *>(blk + 3 * (long) i);
#pragma unroll
      for (int k = 0; k < 6; k++) { const double2 q = s[k]; a[2 * k] = (float) q.x; a[2 * k + 1] = (float) q.y; }
    }
  } else {
    const T *s = blk + 3 * (long) i;
#pragma unroll
    for (int k = 0; k < 12; k++) a[k] = (float) s[k];
  }
}
template <class T, class V>
__device__ inline void store_xyz4(T *__restrict__ blk, int i, const int *__restrict__ user_of, bool wide, const V (&a)[12]) {
  if (user_of) {
    const int4 u = *reinterpret_cast<const int4 *>(user_of + i);
    const int uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; j++) {
      T *d = blk + 3 * (long) uu[j];
      d[0] = (T) a[3 * j]; d[1] = (T) a[3 * j + 1]; d[2] = (T) a[3 * j + 2];
    }
  } else if (wide) {
    if constexpr (sizeof(T) == 4) {
      float4 *d = reinterpret_cast<float4 *>(blk + 3 * (long) i);
      d[0] = make_float4((float) a[0], (float) a[1], (float) a[2], (float) a[3]);
      d[1] = make_float4((float) a[4], (float) a[5], (float) a[6], (float) a[7]);
      d[2] = make_float4((float) a[8], (float) a[9], (float) a[10], (float) a[11]);
    } else {
      double2 *d = reinterpret_cast<double2 *>(blk + 3 * (long) i);
#pragma unroll
      for (int k = 0; k < 6; k++) d[k] = make_double2((double) a[2 * k], (double) a[2 * k + 1]);
    }
  } else {
    T *d = blk + 3 * (long) i;
#pragma unroll
    for (int k = 0; k < 12; k++) d[k] = (T) a[k];
  }
}

// ---- (a) layout conversion of `rows` = slots x rollouts blocks. VEC: n % 4 == 0 and the planar side 16-byte aligned — every plane of
// every block then starts on a 16-byte boundary (planes start at multiples of n floats); total = rows * n / 4 lanes. Else one vertex per lane.
template <class T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_rows_to_planar(const T *__restrict__ src, float *__restrict__ dst, int n, long total,
                                                             const int *__restrict__ user_of, int iwide) {
  const long t = (long) blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  if constexpr (VEC) {
    const int nq = n >> 2;
    const long r = t / nq;
    const int i = (int) (t - r * nq) << 2;
    float a[12];
    load_xyz4(src + r * 3 * n, i, user_of, iwide != 0, a);
    float *d = dst + r * 3 * n + i;
    *reinterpret_cast<float4 *>(d) = make_float4(a[0], a[3], a[6], a[9]);
    *reinterpret_cast<float4 *>(d + n) = make_float4(a[1], a[4], a[7], a[10]);
    *reinterpret_cast<float4 *>(d + 2 * (long) n) = make_float4(a[2], a[5], a[8], a[11]);
  } else {
    const long r = t / n;
    const int i = (int) (t - r * n);
    const T *s = src + (r * n + (user_of ? user_of[i] : i)) * 3;
    float *d = dst + r * 3 * n;
    d[i] = (float) s[0]; d[n + i] = (float) s[1]; d[2 * (long) n + i] = (float) s[2];
  }
}
template <class T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_planar_to_rows(const float *__restrict__ src, T *__restrict__ dst, int n, long total,
                                                             const int *__restrict__ user_of, int iwide) {
  const long t = (long) blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  if constexpr (VEC) {
    const int nq = n >> 2;
    const long r = t / nq;
    const int i = (int) (t - r * nq) << 2;
    const float *s = src + r * 3 * n + i;
    const float4 p0 = *reinterpret_cast<const float4 *>(s), p1 = *reinterpret_cast<const float4 *>(s + n),
                 p2 = *reinterpret_cast<const float4 *>(s + 2 * (long) n);
    const float a[12] = {p0.x, p1.x, p2.x, p0.y, p1.y, p2.y, p0.z, p1.z, p2.z, p0.w, p1.w, p2.w};
    store_xyz4(dst + r * 3 * n, i, user_of, iwide != 0, a);
  } else {
    const long r = t / n;
    const int i = (int) (t - r * n);
    const float *s = src + r * 3 * n;
    T *d = dst + (r * n + (user_of ? user_of[i] : i)) * 3;
    d[0] = (T) s[i]; d[1] = (T) s[n + i]; d[2] = (T) s[2 * (long) n + i];
  }
}

// ---- (b) cast-in of small per-rollout data (uniform forces, factors, mu): the inverse of k_copy_cast
template <class T>
__global__ __launch_bounds__(kThreads) void k_cast_in(const T *__restrict__ src, float *__restrict__ dst, long total) {
  const long t = (long) blockIdx.x * kThreads + threadIdx.x;
  if (t < total) dst[t] = (float) src[t];
}

// ---- (c) force-schedule gradients from the kept y tape. Sums run in fp64 in a fixed order (lane-strided partial sums, wave shuffle tree,
// the waves' sums added in wave order) and are rounded once, to the output type; no atomics: bit-reproducible from run to run.
__device__ inline double block_sum(double v) {
  __shared__ double part[kThreads / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kThreads / 64; w++) s += part[w];
  return s;     // valid in thread 0
}
// dL/dfv_scale[k][b] = h^2 sum_{d, i} y[k][b][d][i] fv[b][d][i]: one workgroup per (slot, rollout); both operands planar in device numbering
template <class T>
__global__ __launch_bounds__(kThreads) void k_dfv_scale(const float *__restrict__ ys, const float *__restrict__ fv, T *__restrict__ out, int B,
                                                        long n3, double h2, int wide) {
  const long row = blockIdx.x;
  const float *y = ys + row * n3, *f = fv + (row % B) * n3;
  double acc = 0;
  if (wide) {
    const float4 *y4 = reinterpret_cast<const float4 *>(y), *f4 = reinterpret_cast<const float4 *>(f);
    for (long q = threadIdx.x; q < (n3 >> 2); q += kThreads) {
      const float4 a = y4[q], c = f4[q];
      acc += (double) a.x * (double) c.x; acc += (double) a.y * (double) c.y; acc += (double) a.z * (double) c.z; acc += (double) a.w * (double) c.w;
    }
  } else {
    for (long q = threadIdx.x; q < n3; q += kThreads) acc += (double) y[q] * (double) f[q];
  }
  acc = block_sum(acc);
  if (threadIdx.x == 0) out[row] = (T) (h2 * acc);
}
// dL/dfv[b][i][d] = h^2 sum_k w[k][b] y[k][b][d][i] (w null: factor 1), written interleaved in the caller's numbering
template <class T, bool VEC>
__global__ __launch_bounds__(kThreads) void k_dfv(const float *__restrict__ ys, const float *__restrict__ w, T *__restrict__ out, int B, int n,
                                                  int nslots, long total, const int *__restrict__ user_of, int iwide, double h2) {
  const long t = (long) blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const long slot_stride = (long) B * 3 * n;
  if constexpr (VEC) {
    const int nq = n >> 2;
    const long b = t / nq;
    const int i = (int) (t - b * nq) << 2;
    double acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < nslots; k++) {
      const float *s = ys + k * slot_stride + b * 3 * n + i;
      const double wk = w ? (double) w[(long) k * B + b] : 1.0;
      const float4 p0 = *reinterpret_cast<const float4 *>(s), p1 = *reinterpret_cast<const float4 *>(s + n),
                   p2 = *reinterpret_cast<const float4 *>(s + 2 * (long) n);
      acc[0] += wk * p0.x; acc[1] += wk * p1.x; acc[2] += wk * p2.x; acc[3] += wk * p0.y; acc[4] += wk * p1.y; acc[5] += wk * p2.y;
      acc[6] += wk * p0.z; acc[7] += wk * p1.z; acc[8] += wk * p2.z; acc[9] += wk * p0.w; acc[10] += wk * p1.w; acc[11] += wk * p2.w;
    }
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] *= h2;
    store_xyz4(out + b * 3 * n, i, user_of, iwide != 0, acc);
  } else {
    const long b = t / n;
    const int i = (int) (t - b * n);
    double a0 = 0, a1 = 0, a2 = 0;
    for (int k = 0; k < nslots; k++) {
      const float *s = ys + k * slot_stride + b * 3 * n;
      const double wk = w ? (double) w[(long) k * B + b] : 1.0;
      a0 += wk * s[i]; a1 += wk * s[n + i]; a2 += wk * s[2 * (long) n + i];
    }
    T *d = out + (b * n + (user_of ? user_of[i] : i)) * 3;
    d[0] = (T) (h2 * a0); d[1] = (T) (h2 * a1); d[2] = (T) (h2 * a2);
  }
}
// dL/dfu[k][b][0..2] = elements 4 .. 6 of the step's parameter gradients ([slots][B][8]; they hold h^2 sum_i y_i already)
template <class T>
__global__ __launch_bounds__(kThreads) void k_dfu(const float *__restrict__ dpar, T *__restrict__ out, long total) {
  const long t = (long) blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const long r = t / 3;
  out[t] = (T) dpar[r * 8 + 4 + (t - r * 3)];
}

// ---- (d) primitive centres of `rows` = slots x rollouts from per-group offsets d[rows][G][3] (null: none): one lane per (row, flattened
// primitive), the rule of dc_primoffset.h — fp64 sum of the built centre and the offset of the primitive's group, rounded once
template <class T>
__global__ __launch_bounds__(kThreads) void k_prim_centres(const double *__restrict__ built, const int *__restrict__ group_of_prim, const T *__restrict__ d,
                                                           float *__restrict__ dst, int P, int G, long total) {
  const long t = (long) blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const long r = t / P;
  const int p = (int) (t - r * P);
  const T *dr = d ? d + (r * G + group_of_prim[p]) * 3 : nullptr;
#pragma unroll
  for (int k = 0; k < 3; k++) dst[t * 3 + k] = offset_centre(built[3 * p + k], dr ? (double) dr[k] : 0.0);
}

}  // namespace

void launch_prim_centres(const double *built, const int *group_of_prim, const void *d, int is_f32, float *dst, long rows, int P, int G, hipStream_t st) {
  const long total = rows * P;
  if (total <= 0) return;
  const dim3 g(blocks_for(total)), b(kThreads);
  if (is_f32) hipLaunchKernelGGL(k_prim_centres<float>, g, b, 0, st, built, group_of_prim, (const float *) d, dst, P, G, total);
  else hipLaunchKernelGGL(k_prim_centres<double>, g, b, 0, st, built, group_of_prim, (const double *) d, dst, P, G, total);
}

void launch_rows_to_planar(const void *src, int is_f32, float *dst, long rows, int n, const int *user_of, hipStream_t st) {
  if (rows <= 0 || n <= 0) return;
  const bool vec = (n & 3) == 0 && aligned16(dst);
  const int iwide = vec && !user_of && aligned16(src);
  const long total = vec ? rows * (n >> 2) : rows * n;
  const dim3 g(blocks_for(total)), b(kThreads);
  if (is_f32) {
    if (vec) hipLaunchKernelGGL((k_rows_to_planar<float, true>), g, b, 0, st, (const float *) src, dst, n, total, user_of, iwide);
    else hipLaunchKernelGGL((k_rows_to_planar<float, false>), g, b, 0, st, (const float *) src, dst, n, total, user_of, 0);
  } else {
    if (vec) hipLaunchKernelGGL((k_rows_to_planar<double, true>), g, b, 0, st, (const double *) src, dst, n, total, user_of, iwide);
    else hipLaunchKernelGGL((k_rows_to_planar<double, false>), g, b, 0, st, (const double *) src, dst, n, total, user_of, 0);
  }
}
void launch_planar_to_rows(const float *src, void *dst, int is_f32, long rows, int n, const int *user_of, hipStream_t st) {
  if (rows <= 0 || n <= 0) return;
  const bool vec = (n & 3) == 0 && aligned16(src);
  const int iwide = vec && !user_of && aligned16(dst);
  const long total = vec ? rows * (n >> 2) : rows * n;
  const dim3 g(blocks_for(total)), b(kThreads);
  if (is_f32) {
    if (vec) hipLaunchKernelGGL((k_planar_to_rows<float, true>), g, b, 0, st, src, (float *) dst, n, total, user_of, iwide);
    else hipLaunchKernelGGL((k_planar_to_rows<float, false>), g, b, 0, st, src, (float *) dst, n, total, user_of, 0);
  } else {
    if (vec) hipLaunchKernelGGL((k_planar_to_rows<double, true>), g, b, 0, st, src, (double *) dst, n, total, user_of, iwide);
    else hipLaunchKernelGGL((k_planar_to_rows<double, false>), g, b, 0, st, src, (double *) dst, n, total, user_of, 0);
  }
}
void launch_cast_in(const void *src, int is_f32, float *dst, long total, hipStream_t st) {
  if (total <= 0) return;
  if (is_f32) hipLaunchKernelGGL(k_cast_in<float>, dim3(blocks_for(total)), dim3(kThreads), 0, st, (const float *) src, dst, total);
  else hipLaunchKernelGGL(k_cast_in<double>, dim3(blocks_for(total)), dim3(kThreads), 0, st, (const double *) src, dst, total);
}
void launch_dfu_from_param(const float *dpar, void *out, int is_f32, long rows, hipStream_t st) {
  const long total = rows * 3;
  if (total <= 0) return;
  if (is_f32) hipLaunchKernelGGL(k_dfu<float>, dim3(blocks_for(total)), dim3(kThreads), 0, st, dpar, (float *) out, total);
  else hipLaunchKernelGGL(k_dfu<double>, dim3(blocks_for(total)), dim3(kThreads), 0, st, dpar, (double *) out, total);
}
void launch_dfv_scale(const float *ys, const float *fv, void *out, int is_f32, int nslots, int B, int N, double h2, hipStream_t st) {
  const long rows = (long) nslots * B, n3 = 3 * (long) N;
  if (rows <= 0 || n3 <= 0) return;
  const int wide = (n3 & 3) == 0 && aligned16(ys) && aligned16(fv);
  if (is_f32) hipLaunchKernelGGL(k_dfv_scale<float>, dim3((unsigned) rows), dim3(kThreads), 0, st, ys, fv, (float *) out, B, n3, h2, wide);
  else hipLaunchKernelGGL(k_dfv_scale<double>, dim3((unsigned) rows), dim3(kThreads), 0, st, ys, fv, (double *) out, B, n3, h2, wide);
}
void launch_dfv(const float *ys, const float *w, void *out, int is_f32, int nslots, int B, int N, const int *user_of, double h2, hipStream_t st) {
  if (nslots <= 0 || B <= 0 || N <= 0) return;
  const bool vec = (N & 3) == 0 && aligned16(ys);
  const int iwide = vec && !user_of && aligned16(out);
  const long total = vec ? (long) B * (N >> 2) : (long) B * N;
  const dim3 g(blocks_for(total)), b(kThreads);
  if (is_f32) {
    if (vec) hipLaunchKernelGGL((k_dfv<float, true>), g, b, 0, st, ys, w, (float *) out, B, N, nslots, total, user_of, iwide, h2);
    else hipLaunchKernelGGL((k_dfv<float, false>), g, b, 0, st, ys, w, (float *) out, B, N, nslots, total, user_of, 0, h2);
  } else {
    if (vec) hipLaunchKernelGGL((k_dfv<double, true>), g, b, 0, st, ys, w, (double *) out, B, N, nslots, total, user_of, iwide, h2);
    else hipLaunchKernelGGL((k_dfv<double, false>), g, b, 0, st, ys, w, (double *) out, B, N, nslots, total, user_of, 0, h2);
  }
}

}  // namespace dc
