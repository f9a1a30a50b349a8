// GPU check library of the dense adjoint solve's LU (tests/test_gpu_dense_lu.py): the product's own translation unit, included as text, so
// launch_dense_factor (k_lu_panel, k_lu_trsm, k_lu_update), lu_substitute<1024> and DenseAdjWork are exactly what the engine runs, on
// matrices a scene cannot produce. Built by diffcloth_amd/build.py (build_kernel_checks) into diffcloth_amd/lib/libdc_dense_lu_check.so.
#include "../../diffcloth_amd/csrc/dc_adjoint_dense.hip"

#include <cstdio>
#include <cstring>

namespace dc {
namespace {

// x = K^-1 rhs with the factors of matrix blockIdx.y, right-hand side blockIdx.x: bv and blk in LDS as in k_adjoint_dense_step
__global__ __launch_bounds__(1024) void k_check_substitute(DenseAdjWork D, int n, int nrhs, const double *__restrict__ rhs, double *__restrict__ x) {
  __shared__ double bv[3 * kDenseMaxN], blk[kLuPanel * kLuPanel];
  const int m = blockIdx.y, tid = threadIdx.x;
  if (D.flag[m]) return;
  const size_t off = ((size_t) m * nrhs + blockIdx.x) * n;
  for (int q = tid; q < n; q += 1024) bv[q] = rhs[off + q];
  __syncthreads();
  lu_substitute<1024>(D.K + (size_t) m * D.ld * D.ld, D.piv + (size_t) m * D.ld, n, (size_t) D.ld, bv, blk);
  for (int q = tid; q < n; q += 1024) x[off + q] = bv[q];
}

}  // namespace
}  // namespace dc

namespace {

struct Bufs {
  void *p[5] = {};
  ~Bufs() { for (void *q : p) if (q) (void) hipFree(q); }
};

int fail(char *err, int errlen, const char *what, hipError_t e) {
  if (err && errlen > 0) snprintf(err, (size_t) errlen, "%s: %s", what, hipGetErrorString(e));
  return 1;
}

}  // namespace

#define CHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(err, errlen, #call, e_); } while (0)

// nb column-major n x n matrices of leading dimension ld (K [nb][ld][ld], every entry uploaded, padding included), piv [nb][ld] and
// flag [nb] as the caller filled them, nrhs right-hand sides per matrix (rhs, x [nb][nrhs][n]). On return K holds the factors in place,
// piv the pivot rows, flag the singular / non-finite marks, x the solutions (x of a flagged matrix is left as the caller filled it).
// Returns 0, or 1 with a message in err.
extern "C" int dc_check_dense_lu(int nb, int n, int ld, double *K, int *piv, int *flag, int nrhs, const double *rhs, double *x, char *err, int errlen) {
  if (nb < 1 || n < 1 || n > 3 * dc::kDenseMaxN || ld < n || nrhs < 0 || !K || !piv || !flag || (nrhs && (!rhs || !x))) {
    if (err && errlen > 0) snprintf(err, (size_t) errlen, "dc_check_dense_lu: bad arguments");
    return 1;
  }
  const size_t kbytes = (size_t) nb * ld * ld * sizeof(double), pbytes = (size_t) nb * ld * sizeof(int), fbytes = (size_t) nb * sizeof(int);
  const size_t vbytes = (size_t) nb * nrhs * n * sizeof(double);
  Bufs B;
  dc::DenseAdjWork D{};
  CHK(hipMalloc(&B.p[0], kbytes)); CHK(hipMalloc(&B.p[1], pbytes)); CHK(hipMalloc(&B.p[2], fbytes));
  D.K = (double *) B.p[0]; D.piv = (int *) B.p[1]; D.flag = (int *) B.p[2]; D.ld = ld;
  CHK(hipMemcpy(D.K, K, kbytes, hipMemcpyHostToDevice));
  CHK(hipMemcpy(D.piv, piv, pbytes, hipMemcpyHostToDevice));
  CHK(hipMemcpy(D.flag, flag, fbytes, hipMemcpyHostToDevice));
  dc::launch_dense_factor(D, n, nb, nullptr);
  CHK(hipGetLastError());
  if (nrhs) {
    CHK(hipMalloc(&B.p[3], vbytes)); CHK(hipMalloc(&B.p[4], vbytes));
    CHK(hipMemcpy(B.p[3], rhs, vbytes, hipMemcpyHostToDevice));
    CHK(hipMemcpy(B.p[4], x, vbytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(dc::k_check_substitute, dim3(nrhs, nb), dim3(1024), 0, nullptr, D, n, nrhs, (const double *) B.p[3], (double *) B.p[4]);
    CHK(hipGetLastError());
  }
  CHK(hipDeviceSynchronize());
  CHK(hipMemcpy(K, D.K, kbytes, hipMemcpyDeviceToHost));
  CHK(hipMemcpy(piv, D.piv, pbytes, hipMemcpyDeviceToHost));
  CHK(hipMemcpy(flag, D.flag, fbytes, hipMemcpyDeviceToHost));
  if (nrhs) CHK(hipMemcpy(x, B.p[4], vbytes, hipMemcpyDeviceToHost));
  return 0;
}
