// GPU check library of the band adjoint solve's LU (tests/test_gpu_band_lu.py): the product's own translation unit, included as text, so
// launch_band_factor (k_band_panel, k_band_trsm, k_band_update), band_substitute<1024> and BandAdjWork are exactly what the engine runs, on
// band matrices a scene cannot produce. Built by diffcloth_amd/build.py (build_kernel_checks) into diffcloth_amd/lib/libdc_band_lu_check.so.
#include "../../diffcloth_amd/csrc/dc_adjoint_band.hip"

#include <cstdio>
#include <cstring>

namespace dc {

// launch_band_assemble (not called here) refers to the dense solve's prep launcher, which lives in another translation unit: a stub
// keeps this library to the code under test
void launch_dense_prep(const DevSystem &, const BwdArgs &, double *, const DenseAdjWork &, int, int, hipStream_t) {}

namespace {

// x = K^-1 rhs with the factors of band blockIdx.y, right-hand side blockIdx.x: bv and blk in dynamic LDS as in k_adjoint_band_step
__global__ __launch_bounds__(1024) void k_check_band_substitute(BandAdjWork D, int nrhs, const double *__restrict__ rhs, double *__restrict__ x) {
  extern __shared__ __attribute__((aligned(16))) double dyn[];
  const int m = blockIdx.y, tid = threadIdx.x, n = D.n;
  if (D.flag[m]) return;
  double *bv = dyn, *blk = dyn + band_round16(n);      // blk [band_blk_doubles(kl, sub_cols)]
  const size_t off = ((size_t) m * nrhs + blockIdx.x) * n;
  for (int q = tid; q < n; q += 1024) bv[q] = rhs[off + q];
  __syncthreads();
  band_substitute<1024>(D.AB + (size_t) m * D.ldab * n, D.piv + (size_t) m * D.npiv, n, D.kl, (size_t) D.ldab, D.sub_cols, bv, blk);
  for (int q = tid; q < n; q += 1024) x[off + q] = bv[q];
}

}  // namespace
}  // namespace dc

namespace {

struct Bufs {
  void *p[6] = {};
  ~Bufs() { for (void *q : p) if (q) (void) hipFree(q); }
};

int fail(char *err, int errlen, const char *what, hipError_t e) {
  if (err && errlen > 0) snprintf(err, (size_t) errlen, "%s: %s", what, hipGetErrorString(e));
  return 1;
}

}  // namespace

#define CHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(err, errlen, #call, e_); } while (0)

// nb band matrices of order n with kl = ku sub- and super-diagonals in LAPACK band storage of leading dimension ldab >= 3 kl + 1
// (AB [nb][n][ldab], element (r, c) at (2 kl + r - c) + c ldab, every entry uploaded, padding included; the kl fill rows zero), piv [nb][npiv]
// and flag [nb] as the caller filled them, nrhs right-hand sides per matrix (rhs, x [nb][nrhs][n]). On return AB holds the factors in place
// (dc_adjoint_band.h), piv the pivot rows, flag the singular / non-finite marks, x the solutions (x of a flagged matrix is left as the
// caller filled it). Returns 0, or 1 with a message in err.
extern "C" int dc_check_band_lu(int nb, int n, int kl, int ldab, int npiv, double *AB, int *piv, int *flag, int nrhs, const double *rhs, double *x,
                                char *err, int errlen) {
  const int cols = dc::band_sub_cols((n + 2) / 3, kl);
  const long long lds = (long long) sizeof(double) * ((long long) dc::band_round16(n) + dc::band_blk_doubles(kl, cols));
  if (nb < 1 || n < 1 || kl < 0 || kl > n - 1 + (n == 1) || ldab < 3 * kl + 1 || npiv < n || nrhs < 0 || !AB || !piv || !flag || (nrhs && (!rhs || !x)) ||
      cols < 1 || lds > dc::kBandLdsBytes) {
    if (err && errlen > 0) snprintf(err, (size_t) errlen, "dc_check_band_lu: bad arguments");
    return 1;
  }
  const size_t abytes = (size_t) nb * ldab * n * sizeof(double), pbytes = (size_t) nb * npiv * sizeof(int), fbytes = (size_t) nb * sizeof(int);
  const size_t vbytes = (size_t) nb * nrhs * n * sizeof(double);
  Bufs B;
  dc::BandAdjWork D{};
  D.n = n; D.kl = kl; D.ldab = ldab; D.pld = dc::band_pld(kl); D.npiv = npiv; D.sub_cols = cols;
  CHK(hipMalloc(&B.p[0], abytes)); CHK(hipMalloc(&B.p[1], pbytes)); CHK(hipMalloc(&B.p[2], fbytes));
  CHK(hipMalloc(&B.p[5], (size_t) nb * 2 * dc::kBandPanel * D.pld * sizeof(double)));
  D.AB = (double *) B.p[0]; D.piv = (int *) B.p[1]; D.flag = (int *) B.p[2]; D.panel = (double *) B.p[5];
  CHK(hipMemcpy(D.AB, AB, abytes, hipMemcpyHostToDevice));
  CHK(hipMemcpy(D.piv, piv, pbytes, hipMemcpyHostToDevice));
  CHK(hipMemcpy(D.flag, flag, fbytes, hipMemcpyHostToDevice));
  CHK(dc::launch_band_factor(D, nb, nullptr, nullptr));
  CHK(hipGetLastError());
  if (nrhs) {
    CHK(hipMalloc(&B.p[3], vbytes)); CHK(hipMalloc(&B.p[4], vbytes));
    CHK(hipMemcpy(B.p[3], rhs, vbytes, hipMemcpyHostToDevice));
    CHK(hipMemcpy(B.p[4], x, vbytes, hipMemcpyHostToDevice));
    CHK(dc::ensure_dynamic_lds<dc::k_check_band_substitute>((size_t) lds));
    hipLaunchKernelGGL(dc::k_check_band_substitute, dim3(nrhs, nb), dim3(1024), (size_t) lds, nullptr, D, nrhs, (const double *) B.p[3], (double *) B.p[4]);
    CHK(hipGetLastError());
  }
  CHK(hipDeviceSynchronize());
  CHK(hipMemcpy(AB, D.AB, abytes, hipMemcpyDeviceToHost));
  CHK(hipMemcpy(piv, D.piv, pbytes, hipMemcpyDeviceToHost));
  CHK(hipMemcpy(flag, D.flag, fbytes, hipMemcpyDeviceToHost));
  if (nrhs) CHK(hipMemcpy(x, B.p[4], vbytes, hipMemcpyDeviceToHost));
  return 0;
}
