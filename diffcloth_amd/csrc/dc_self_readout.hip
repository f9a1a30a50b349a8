// Self-contact read-out (dc_get_self_contact_readout / dc_get_self_contact_readout_dev): what the cloth's sheets press on each other with,
// re-formed on the device from the tape. include/diffcloth_hip.h states the rule; in short, per record:
//   g_i = f_i + r_p,i at the vertices of the record's working set (r_p re-formed as k_contact_readout re-forms it), then layer by layer, per
//   pair k = (A, B): d_k = g_A / m_A - g_B / m_B, r_k = dry_friction(n_k, d_k, kClothMu) / (1/m_A + 1/m_B), g_A += r_k, g_B -= r_k
// with the device functions and the fp32 expressions of self_friction_layers_lds_v (dc_devlib.h). The record's dvec and R are neither read nor
// written.
//
// One workgroup per (slot, rollout) row, every row of the launch in ONE launch. The working set is the record's own (SelfRec::verts, slots in
// nrm.w): f, g - f and 1 / m of its M vertices, the per-vertex fp64 sums, the contacts' normals and the layer offsets live in LDS
// (dc_self_readout.h has the image). Up to kWideLayers layers the whole workgroup takes the pairs of a layer, with a barrier per layer; beyond
// that ONE wave walks the layers in program order behind the wavefront fence (the tested stacks: 193 ... 524 layers). A row whose image does
// not fit `lds_floats` takes the same walk in global memory (g - f in the scratch planes, a barrier per layer, the form of
// self_friction_layers_v) with the SAME assignment of pairs to lanes, so that both paths sum in one order and give the same bits.
// The lane that evaluates a pair writes its layer, state and impulse; the pair's two ids are a copy and go out in a parallel pass.
// Sums: per vertex in fp64 in layer order (a vertex is in at most one pair of a layer); totals as lane partial sums in fp64, wave shuffle tree,
// the waves' sums added in wave order. No atomics: bit-reproducible.
// Traffic model per row: 16 B normal + 8 B ids per contact, 4 (vertex) + 12 (f) + 4 (prim) + 4 (mass) B per working-set vertex, 12 B more (the
// primitive normal) where that vertex is in primitive contact, 4 B per layer, plus what is written.
#define DC_KERNEL_TU
#include "dc_devlib.h"
#include "dc_launch.h"
#include "dc_self_readout.h"

namespace dc {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSums = 5;      // sum jn, sum |r_T|, take-off, stick, slide

// a floating output array of the caller's type, element alignment only
struct Out {
  void *p;
  int f32;
  __device__ __forceinline__ Out at(long i) const { return Out{p ? (f32 ? (void *) ((float *) p + i) : (void *) ((double *) p + i)) : nullptr, f32}; }
  __device__ __forceinline__ void st(long i, double v) const { if (f32) ((float *) p)[i] = (float) v; else ((double *) p)[i] = v; }
};

// the working set in LDS, indexed by working-set slot
struct LdsSet {
  float *f, *r, *im;
  double *s;
  int M;
  __device__ __forceinline__ f3 ldf(int i) const { return mk(f[i], f[M + i], f[2 * M + i]); }
  __device__ __forceinline__ f3 ldr(int i) const { return mk(r[i], r[M + i], r[2 * M + i]); }
  __device__ __forceinline__ void str(int i, f3 v) const { r[i] = v.x; r[M + i] = v.y; r[2 * M + i] = v.z; }
  __device__ __forceinline__ float inv_mass(int i) const { return im[i]; }
  __device__ __forceinline__ void add(int i, double x, double y, double z) const { s[i] += x; s[M + i] += y; s[2 * M + i] += z; }
};
// the working set in global memory, indexed by vertex
struct GlobalSet {
  const float *f;
  float *r;
  const float DC_G *mass;
  double *s;
  int N;
  __device__ __forceinline__ f3 ldf(int i) const { return ld3(f, i, N); }
  __device__ __forceinline__ f3 ldr(int i) const { return mk(r[i], r[N + i], r[2 * N + i]); }
  __device__ __forceinline__ void str(int i, f3 v) const { r[i] = v.x; r[N + i] = v.y; r[2 * N + i] = v.z; }
  __device__ __forceinline__ float inv_mass(int i) const { return 1.0f / mass[i]; }
  __device__ __forceinline__ void add(int i, double x, double y, double z) const { s[i] += x; s[N + i] += y; s[2 * N + i] += z; }
};

// pair k of layer l between the entries ia and ib of the working set W: the step's expressions (self_friction_layers_lds_v), the outputs of
// the pair, the lane's partial sums
template <class W>
__device__ __forceinline__ void eval_pair(const W &w, int ia, int ib, f3 n, int k, int l, int cap_out, int *pairs, const Out &impulse, double *acc) {
  const float iA = w.inv_mass(ia), iB = w.inv_mass(ib);
  f3 rA = w.ldr(ia), rB = w.ldr(ib);
  const f3 d = (w.ldf(ia) + rA) * iA - (w.ldf(ib) + rB) * iB;
  const f3 ri = dry_friction(n, d, kClothMu) * (1.0f / (iA + iB));           // k = mA mB / (mA + mB)
  const int st = contact_state(n, d, kClothMu);
  w.str(ia, rA + ri);
  w.str(ib, rB - ri);
  const double rx = ri.x, ry = ri.y, rz = ri.z;
  w.add(ia, rx, ry, rz);
  w.add(ib, -rx, -ry, -rz);
  const double jn = rx * (double) n.x + ry * (double) n.y + rz * (double) n.z;
  const double tx = rx - jn * (double) n.x, ty = ry - jn * (double) n.y, tz = rz - jn * (double) n.z;
  acc[0] += jn;
  acc[1] += sqrt(tx * tx + ty * ty + tz * tz);
  acc[2] += st == 1; acc[3] += st == 2; acc[4] += st == 3;
  if (k < cap_out) {
    if (pairs) { pairs[4 * (long) k + 2] = l; pairs[4 * (long) k + 3] = st; }
    if (impulse.p) { impulse.st(4 * (long) k, rx); impulse.st(4 * (long) k + 1, ry); impulse.st(4 * (long) k + 2, rz); impulse.st(4 * (long) k + 3, jn); }
  }
}

}  // namespace

// ONE instance serves both output types (`f32`: the floating outputs are float, else double): the type matters at the stores only, so the
// fp32 and the fp64 form of a call run the same instructions and agree bit for bit up to the cast.
__global__ __launch_bounds__(kThreads) void k_self_readout(const DevSystem *__restrict__ Sp, const SelfRoArgs A, int *__restrict__ pairs_out,
                                                           void *__restrict__ impulse_out, void *__restrict__ vimp_out, void *__restrict__ totals_out,
                                                           const int f32) {
  extern __shared__ float4 dyn4[];
  __shared__ double part[kWaves][kSums];
  const DevSystem &S = *Sp;
  const int N = S.N, G = S.ngroups, cap = S.self_cap, tid = threadIdx.x;
  const long row = A.row0 + (long) blockIdx.x;
  const int b = (int) (row % A.B);
  const float *f = A.F + row * 3 * N, *nr = A.NRM + row * 3 * N;
  const int *pr = A.PRIM + row * N;
  const float *wv = A.PV ? A.PV + row * G * kPvRow : nullptr;
  const float *mub = A.mu + (long) b * G;
  const int DC_G *user_of = S.user_of;
  const int *meta = A.R.meta + row * kMetaStride;
  const int2 *pair = A.R.pair + row * cap;
  const float4 *nrm = A.R.nrm + row * cap;
  const int *verts = A.R.verts + row * 2 * cap;
  const int cap_out = A.cap_out;
  int *pairs = pairs_out ? pairs_out + row * 4 * cap_out : nullptr;
  const Out impulse = Out{impulse_out, f32}.at(row * 4 * cap_out), vimp = Out{vimp_out, f32}.at(row * 3 * N);

  // a context without self-collision has no list (the step kernels read none either); the sizes of a list are held to what the context can hold
  const bool on = S.contact_enabled && S.self_enabled;
  const int M = on && meta[0] > 0 ? min(max(meta[kMetaStride - 1], 0), min(N, 2 * cap)) : 0;
  const int C = M >= 2 ? min(meta[0], cap) : 0;       // (a pair has two distinct vertices)
  const int nl = C ? min(max(meta[1], 0), kMaxLayers) : 0;
  const bool fits = selfro_lds_need(M, C, nl) <= A.lds_floats;     // (when it does not, the host's plan has given the launch its scratch: dc_self_readout.h)
  const int stride = nl <= kWideLayers ? kThreads : 64;           // lanes that take the pairs of a layer, on both paths

  // everything that is not a contact's: zeros in the caller's vertex rows, the padding behind the list, the ids of the listed pairs
  if (vimp.p) for (int e = tid; e < 3 * N; e += kThreads) vimp.st(e, 0.0);
  for (int c = min(C, cap_out) + tid; c < cap_out; c += kThreads) {
    if (pairs) { int *o = pairs + 4 * (long) c; o[0] = -1; o[1] = -1; o[2] = -1; o[3] = 0; }
    if (impulse.p) for (int q = 0; q < 4; q++) impulse.st(4 * (long) c + q, 0.0);
  }
  if (pairs)
    for (int c = tid; c < min(C, cap_out); c += kThreads) {
      const int2 ab = pair[c];
      pairs[4 * (long) c] = user_of ? user_of[ab.x] : ab.x;
      pairs[4 * (long) c + 1] = user_of ? user_of[ab.y] : ab.y;
    }
  // r_p of vertex v, as k_contact_readout re-forms it
  auto prim_part = [&](int v, f3 fv) {
    const int prim = pr[v];
    if (prim < 0) return mk(0, 0, 0);
    const f3 n = ld3(nr, v, N);
    return dry_friction(n, prim_d(S.prims[prim], n, fv, S.mass[v], wv), mub[S.prims[prim].group]);
  };

  double acc[kSums] = {0, 0, 0, 0, 0};
  if (fits) {
    float *lds = (float *) dyn4;
    const float4 *ln = dyn4;
    LdsSet w;
    w.s = (double *) (lds + 4 * C); w.f = lds + 4 * C + 6 * M; w.r = w.f + 3 * M; w.im = w.r + 3 * M; w.M = M;
    int *loff = (int *) (w.im + M);
    for (int s = tid; s < M; s += kThreads) {
      const int v = verts[s];
      const f3 fv = ld3(f, v, N);
      w.f[s] = fv.x; w.f[M + s] = fv.y; w.f[2 * M + s] = fv.z;
      w.str(s, prim_part(v, fv));
      w.im[s] = 1.0f / S.mass[v];
      w.s[s] = 0; w.s[M + s] = 0; w.s[2 * M + s] = 0;
    }
    for (int k = tid; k < C; k += kThreads) dyn4[k] = nrm[k];
    for (int l = tid; l <= nl; l += kThreads) loff[l] = min(max(meta[2 + l], 0), C);
    __syncthreads();
    auto contact = [&](int k, int l) {
      const float4 n4 = ln[k];
      const int sl = __float_as_int(n4.w);
      eval_pair(w, min(sl & 0xffff, M - 1), min((sl >> 16) & 0xffff, M - 1), mk(n4.x, n4.y, n4.z), k, l, cap_out, pairs, impulse, acc);
    };
    if (stride == kThreads) {
      for (int l = 0; l < nl; l++) {
        const int k1 = loff[l + 1];
        for (int k = loff[l] + tid; k < k1; k += kThreads) contact(k, l);
        __syncthreads();
      }
    } else {
      if (tid < 64) {
        for (int l = 0; l < nl; l++) {
          const int k1 = loff[l + 1];
          for (int k = loff[l] + tid; k < k1; k += 64) contact(k, l);
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");             // compiler: keep the layers' LDS accesses in order
        }
      }
      __syncthreads();
    }
    if (vimp.p)
      for (int s = tid; s < M; s += kThreads) {
        const int v = verts[s];
        const long o = 3 * (long) (user_of ? user_of[v] : v);
        vimp.st(o, w.s[s]); vimp.st(o + 1, w.s[M + s]); vimp.st(o + 2, w.s[2 * M + s]);
      }
  } else {
    GlobalSet w;
    w.f = f; w.r = A.scratch + (long) b * 3 * N; w.mass = S.mass; w.s = A.sums + (long) b * 3 * N; w.N = N;
    for (int s = tid; s < M; s += kThreads) {
      const int v = verts[s];
      w.str(v, prim_part(v, ld3(f, v, N)));
      w.s[v] = 0; w.s[N + v] = 0; w.s[2 * N + v] = 0;
    }
    __syncthreads();
    for (int l = 0; l < nl; l++) {
      const int k0 = min(max(meta[2 + l], 0), C), k1 = min(max(meta[2 + l + 1], 0), C);
      if (tid < stride)
        for (int k = k0 + tid; k < k1; k += stride) {
          const int2 ab = pair[k];
          const float4 n4 = nrm[k];
          eval_pair(w, ab.x, ab.y, mk(n4.x, n4.y, n4.z), k, l, cap_out, pairs, impulse, acc);
        }
      __syncthreads();
    }
    if (vimp.p)
      for (int s = tid; s < M; s += kThreads) {
        const int v = verts[s];
        const long o = 3 * (long) (user_of ? user_of[v] : v);
        vimp.st(o, w.s[v]); vimp.st(o + 1, w.s[N + v]); vimp.st(o + 2, w.s[2 * N + v]);
      }
  }

  if (!totals_out) return;
#pragma unroll
  for (int k = 0; k < kSums; k++) {
    double v = acc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) part[tid >> 6][k] = v;
  }
  __syncthreads();
  if (tid < kSelfRoTotals) {
    double s = tid == 0 ? C : tid == 1 ? nl : M;
    if (tid >= 3) {
      s = 0;
      for (int wvi = 0; wvi < kWaves; wvi++) s += part[wvi][tid - 3];
    }
    Out{totals_out, f32}.st(row * kSelfRoTotals + tid, s);
  }
}

hipError_t launch_self_readout(const DevSystem &S, const SelfRoArgs &A, long rows, int *pairs, void *impulse, void *vertex_impulse, void *totals,
                               int is_f32, hipStream_t st) {
  if (rows <= 0 || S.N <= 0) return hipSuccess;
  const size_t lds = sizeof(float) * (size_t) A.lds_floats;
  const hipError_t e = ensure_dynamic_lds<k_self_readout>(lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_self_readout, dim3((unsigned) rows), dim3(kThreads), lds, st, S.self_dev, A, pairs, impulse, vertex_impulse, totals, is_f32 ? 1 : 0);
  return hipGetLastError();
}

}  // namespace dc
