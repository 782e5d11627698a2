// mcba_comm_api.hip -- direct RCCL communicators of the C ABI (include/mcba.h, "direct RCCL"): frame-sharded runs all-reduce their
// reduced systems and trial scalars with them.  RCCL is not linked: its entry points are resolved at run time.
#include <dlfcn.h>

#include "mcba_handle.h"

mcba_internal::RcclApi mcba_internal::g_rccl;

using namespace mcba_internal;

static int load_rccl() {
  if (g_rccl.ok) return MCBA_OK;
  void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);
  if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return fail(MCBA_ERR_ARG, "RCCL library not found (dlopen librccl.so)");
  g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
  g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
  g_rccl.AllReduce = reinterpret_cast<decltype(g_rccl.AllReduce)>(dlsym(lib, "ncclAllReduce"));
  g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
  g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
  g_rccl.CommCount = reinterpret_cast<decltype(g_rccl.CommCount)>(dlsym(lib, "ncclCommCount"));
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy) return fail(MCBA_ERR_ARG, "RCCL symbols missing");
  g_rccl.ok = true;
  return MCBA_OK;
}
static int rccl_fail(const char* what, ncclResult_t r) {
  g_err = std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "RCCL error");
  return MCBA_ERR_HIP;
}

extern "C" {

int mcba_comm_unique_id(unsigned char* out128) {
  if (!out128) return fail(MCBA_ERR_ARG, "mcba_comm_unique_id: NULL");
  int rc = load_rccl();
  if (rc) return rc;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  ncclResult_t r = g_rccl.GetUniqueId(&id);
  if (r != ncclSuccess) return rccl_fail("ncclGetUniqueId", r);
  memcpy(out128, &id, 128);
  return MCBA_OK;
}

int mcba_comm_init(mcba_handle* h, const unsigned char* id128, int rank, int world) {
  if (!h || !id128 || world < 1 || rank < 0 || rank >= world) return fail(MCBA_ERR_ARG, "mcba_comm_init: bad argument");
  int rc = load_rccl();
  if (rc) return rc;
  HIPCHK(hipSetDevice(h->device));
  if (h->comm) { g_rccl.CommDestroy(h->comm); h->comm = nullptr; }
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  ncclResult_t r = g_rccl.CommInitRank(&h->comm, world, id, rank);
  if (r != ncclSuccess) { h->comm = nullptr; return rccl_fail("ncclCommInitRank", r); }
  return MCBA_OK;
}

int mcba_comm_allreduce(mcba_handle* h, size_t offset, size_t count) {
  if (!h || !h->comm) return fail(MCBA_ERR_ARG, "mcba_comm_allreduce: no communicator (call mcba_comm_init)");
  NEED_SOLVER(h);   // (the reduce buffer belongs to the lazily allocated solver set)
  if (offset + count > h->nsys + 8 + MCBA_LMS) return fail(MCBA_ERR_ARG, "mcba_comm_allreduce: range outside the reduce buffer");
  ncclResult_t r = g_rccl.AllReduce(h->red + offset, h->red + offset, count, ncclDouble, ncclSum, h->comm, h->stream);
  if (r != ncclSuccess) return rccl_fail("ncclAllReduce", r);
  return MCBA_OK;
}

int mcba_comm_count(mcba_handle* h, int* count) {
  if (!h || !count) return fail(MCBA_ERR_ARG, "mcba_comm_count: bad argument");
  *count = 0;
  if (!h->comm) return MCBA_OK;  // no direct communicator attached
  if (!g_rccl.CommCount) return fail(MCBA_ERR_ARG, "mcba_comm_count: ncclCommCount not available");
  ncclResult_t r = g_rccl.CommCount(h->comm, count);
  if (r != ncclSuccess) return rccl_fail("ncclCommCount", r);
  return MCBA_OK;
}

int mcba_comm_destroy(mcba_handle* h) {
  if (!h) return fail(MCBA_ERR_ARG, "NULL handle");
  if (h->comm && g_rccl.ok) { (void)hipStreamSynchronize(h->stream); g_rccl.CommDestroy(h->comm); }
  h->comm = nullptr;
  return MCBA_OK;
}

}  // extern "C"
