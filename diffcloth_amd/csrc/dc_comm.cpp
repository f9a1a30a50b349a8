// Collective for C++ callers of libdiffcloth_hip.so (the L-BFGS side sums loss + parameter gradients over the ranks):
// dc_comm_unique_id / dc_comm_init / dc_allreduce_sum / dc_comm_destroy of include/diffcloth_hip.h.
// RCCL is bound at run time (dlopen) the first time one of these entry points is used: the library has no link-time and no header dependency on
// it, and a process that already carries an RCCL (torch.distributed) gets that same copy by its soname. The handful of types and constants of its
// C API (rccl.h / nccl.h) the four entry points used here need, restated:
extern "C" {
typedef struct ncclComm *ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclFloat64 = 8 } ncclDataType_t;      // ncclDouble
typedef enum { ncclSum = 0 } ncclRedOp_t;
#define NCCL_UNIQUE_ID_BYTES 128
}
#include <dlfcn.h>
#include <cstring>
#include <string>
#include "dc_context.h"

namespace {
struct RcclApi {
  void *lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  std::string error;
};
RcclApi &rccl() {
  static RcclApi api;
  if (api.lib || !api.error.empty()) return api;
  for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    api.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (api.lib) break;
  }
  if (!api.lib) {
    const char *why = dlerror();      // (one call: dlerror() clears the message it returns)
    api.error = std::string("RCCL not found (dlopen librccl.so.1): ") + (why ? why : "");
    return api;
  }
  api.GetUniqueId = (decltype(api.GetUniqueId)) dlsym(api.lib, "ncclGetUniqueId");
  api.CommInitRank = (decltype(api.CommInitRank)) dlsym(api.lib, "ncclCommInitRank");
  api.AllReduce = (decltype(api.AllReduce)) dlsym(api.lib, "ncclAllReduce");
  api.CommDestroy = (decltype(api.CommDestroy)) dlsym(api.lib, "ncclCommDestroy");
  api.GetErrorString = (decltype(api.GetErrorString)) dlsym(api.lib, "ncclGetErrorString");
  if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy) { api.error = "RCCL library lacks the expected entry points"; api.lib = nullptr; }
  return api;
}
int rccl_fail(dc_ctx *c, const char *what, ncclResult_t r) {
  RcclApi &R = rccl();
  return fail(c, DC_ERR_HIP, std::string(what) + ": " + (R.GetErrorString ? R.GetErrorString(r) : "RCCL error") + " (" + std::to_string((int) r) + ")");
}
}  // namespace

extern "C" {

int dc_comm_unique_id(char *id128) {
  if (!id128) return DC_ERR_INVALID;
  RcclApi &R = rccl();
  if (!R.lib) return DC_ERR_HIP;
  ncclUniqueId id;
  if (R.GetUniqueId(&id) != ncclSuccess) return DC_ERR_HIP;
  std::memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
  return DC_OK;
}

int dc_comm_init(dc_ctx *c, int nranks, int rank, const char *id128) {
  if (!c || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(c, DC_ERR_INVALID, "dc_comm_init: bad arguments");
  if (c->host_only) return fail(c, DC_ERR_STATE, "dc_comm_init: host-only context");
  RcclApi &R = rccl();
  if (!R.lib) return fail(c, DC_ERR_HIP, R.error);
  if (c->comm) { int rc = dc_comm_destroy(c); if (rc) return rc; }
  HIPCHK(c, hipSetDevice(c->device));
  ncclUniqueId id;
  std::memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
  ncclComm_t comm = nullptr;
  ncclResult_t r = R.CommInitRank(&comm, nranks, id, rank);
  if (r != ncclSuccess) return rccl_fail(c, "ncclCommInitRank", r);
  c->comm = (void *) comm; c->comm_ranks = nranks;
  return DC_OK;
}

int dc_allreduce_sum(dc_ctx *c, double *inout, int count) {
  if (!c || !inout || count < 1) return fail(c, DC_ERR_INVALID, "dc_allreduce_sum: bad arguments");
  if (!c->comm) return fail(c, DC_ERR_STATE, "dc_allreduce_sum: dc_comm_init has not been called");
  RcclApi &R = rccl();
  HIPCHK(c, hipSetDevice(c->device));
  double *buf = nullptr;
  HIPCHK(c, hipMalloc((void **) &buf, sizeof(double) * (size_t) count));
  hipError_t e = hipMemcpyAsync(buf, inout, sizeof(double) * (size_t) count, hipMemcpyHostToDevice, c->stream);
  ncclResult_t r = ncclSuccess;
  if (e == hipSuccess) r = R.AllReduce(buf, buf, (size_t) count, ncclFloat64, ncclSum, (ncclComm_t) c->comm, c->stream);
  if (e == hipSuccess && r == ncclSuccess) e = hipMemcpyAsync(inout, buf, sizeof(double) * (size_t) count, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void) hipFree(buf);
  if (r != ncclSuccess) return rccl_fail(c, "ncclAllReduce", r);
  HIPCHK(c, e);
  return DC_OK;
}

int dc_comm_destroy(dc_ctx *c) {
  if (!c) return DC_ERR_INVALID;
  if (!c->comm) return DC_OK;
  RcclApi &R = rccl();
  if (R.lib) (void) R.CommDestroy((ncclComm_t) c->comm);
  c->comm = nullptr; c->comm_ranks = 0;
  return DC_OK;
}

}  // extern "C"
