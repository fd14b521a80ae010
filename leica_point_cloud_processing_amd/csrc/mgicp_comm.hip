// mgicp_comm.hip -- the multi-GPU transports of a context (include/mi355x_gicp.h): the RCCL
// communicator, the node-wide shared row segment and the xGMI row exchange.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <chrono>
#include <cstring>
#include <string>
#include <thread>

#include "mgicp_ctx.hpp"

using namespace mgicp;

// r05 xGMI: end the running totaler (if any) -- it exits when the generation word changes
void mgicp::xgmi_cancel(mgicp_ctx* ctx) {
  if (ctx->have_xgmi && ctx->h_xgen) __atomic_store_n(ctx->h_xgen, ++ctx->xgen, __ATOMIC_RELEASE);
}

// r05: drop the xGMI row exchange (stream drained first: no totaler, no server writes into it)
void mgicp::xgmi_detach(mgicp_ctx* ctx) {
  if (!ctx->have_xgmi) return;
  xgmi_cancel(ctx);
  if (ctx->xstream) (void)hipStreamSynchronize(ctx->xstream);
  for (void* p : ctx->xpeer) (void)hipIpcCloseMemHandle(p);
  ctx->xpeer.clear();
  ctx->xrows.release();
  ctx->have_xgmi = false;
}

extern "C" {

int mgicp_get_unique_id(unsigned char id[128]) {
  if (!id) return MGICP_E_INVALID;
  ncclUniqueId uid;
  if (ncclGetUniqueId(&uid) != ncclSuccess) return MGICP_E_COMM;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  std::memcpy(id, &uid, 128);
  return MGICP_OK;
}

int mgicp_comm_init(mgicp_ctx* ctx, int nranks, int rank, const unsigned char id[128]) {
  if (!ctx || nranks < 1 || rank < 0 || rank >= nranks) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  if (int rj = cov_join_all(ctx)) return rj;  // the shard changes under them
  if (ctx->comm) {
    (void)ncclCommDestroy(ctx->comm);
    ctx->comm = nullptr;
  }
  if (ctx->have_shm) {  // the segment's geometry belongs to the old rank layout
    int rc = sync(ctx);
    if (rc) return rc;
    (void)hipHostUnregister(ctx->shm.base);
    shm::detach(ctx->shm);
    ctx->have_shm = false;
  }
  ctx->nranks = nranks;
  ctx->rank = rank;
  ctx->qperm_valid = false;
  ctx->src_lazy_ready = false;
  ctx->src.have_cov = false;
  ctx->have_corr = false;
  ctx->seed_valid = false;  // the shard (and its per-point match buffers) changes
  ctx->st[kStTransport] = 0;
  // id == NULL: detached shard (debug entry points only, until mgicp_comm_attach_shm).  nranks == 1
  // with an id builds a real one-rank communicator, so the collective code path can be exercised on
  // a single device.
  if (!id) return MGICP_OK;
  ncclUniqueId uid;
  std::memcpy(&uid, id, 128);
  ncclComm_t comm = nullptr;
  const ncclResult_t r = ncclCommInitRank(&comm, nranks, uid, rank);
  if (r != ncclSuccess) {
    // r06: the context stays a detached shard of the same layout (an RCCL-free rank once a segment is
    // attached), so a caller can fall back without re-creating it (parallel.setup_transport)
    return fail(ctx, MGICP_E_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  }
  ctx->comm = comm;
  ctx->st[kStTransport] = 1;
  return MGICP_OK;
}

int mgicp_comm_attach_xgmi(mgicp_ctx* ctx, int on) {
  if (!ctx) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  int rc = cov_join_all(ctx);
  if (rc || (rc = sync(ctx))) return rc;
  xgmi_detach(ctx);
  if (!on) return reset_stamps(ctx);
  if (!ctx->have_shm)
    return fail(ctx, MGICP_E_INVALID, "xGMI row exchange: attach the shared segment first (its rendezvous)");
  if (ctx->nranks - 1 > kMaxPeers) return fail(ctx, MGICP_E_INVALID, "xGMI row exchange: at most 9 ranks");
  // host words of the totaler (pinned, mapped) and its stream, once per context
  if (!ctx->h_xtot) {
    HIPCK(hipHostMalloc(reinterpret_cast<void**>(&ctx->h_xtot), shm::kRowWords * sizeof(unsigned long long) + 64,
                        hipHostMallocMapped | hipHostMallocCoherent));
    HIPCK(hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->d_xtot), ctx->h_xtot, 0));
    std::memset(ctx->h_xtot, 0, shm::kRowWords * sizeof(unsigned long long) + 64);
    ctx->h_xgen = reinterpret_cast<unsigned int*>(ctx->h_xtot + shm::kRowWords);
    ctx->d_xgen = reinterpret_cast<unsigned int*>(ctx->d_xtot + shm::kRowWords);
  }
  if (!ctx->xstream && ctx->aux_stream) {
    if (int rj = cov_join_all(ctx)) return rj;
    ctx->xstream = ctx->aux_stream;
  }
  if (!ctx->xstream) {
    HIPCK(hipStreamCreateWithFlags(&ctx->xstream, hipStreamNonBlocking));
    ctx->xstream_own = true;
  }
  // this rank's exchange buffer, zeroed (stamp 0 is never a pass stamp), published by IPC handle
  const size_t words = 2 * static_cast<size_t>(ctx->shm.max_sup) * shm::kRowWords;
  // fine-grained: peers' servers store into it over xGMI while this rank's totaler polls it
  // inside one running kernel; coarse-grained memory is coherent across devices only at kernel boundaries
  ctx->xrows.fine = true;
  HIPCK(ctx->xrows.reserve(words));
  HIPCK(hipMemset(ctx->xrows.p, 0, ctx->xrows.cap * sizeof(unsigned long long)));
  hipIpcMemHandle_t h;
  static_assert(sizeof(hipIpcMemHandle_t) <= 64, "IPC handle slot");
  HIPCK(hipIpcGetMemHandle(&h, ctx->xrows.p));
  const uint64_t seq = ++ctx->xseq;  // every rank attaches in the same sequence
  std::memcpy(ctx->shm.ipc_handle(ctx->rank), &h, sizeof(h));
  ctx->shm.ipc_flag(ctx->rank)->store(seq, std::memory_order_release);
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < ctx->nranks; ++r) {
    while (ctx->shm.ipc_flag(r)->load(std::memory_order_acquire) < seq) {
      if (shm::elapsed_s(t0) > ctx->remote_deadline_s)
        return fail(ctx, MGICP_E_COMM, "xGMI row exchange: another rank did not publish its buffer");
      std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
  }
  for (int r = 0; r < ctx->nranks; ++r) {
    if (r == ctx->rank) continue;
    hipIpcMemHandle_t hr;
    std::memcpy(&hr, ctx->shm.ipc_handle(r), sizeof(hr));
    void* p = nullptr;
    hipError_t e = hipIpcOpenMemHandle(&p, hr, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) {
      for (void* q : ctx->xpeer) (void)hipIpcCloseMemHandle(q);
      ctx->xpeer.clear();
      return fail(ctx, MGICP_E_HIP, std::string("xGMI row exchange: hipIpcOpenMemHandle: ") + hipGetErrorString(e));
    }
    ctx->xpeer.push_back(p);
  }
  ctx->have_xgmi = true;
  ctx->st[kStTransport] = ctx->comm ? 5 : 4;
  return reset_stamps(ctx);  // every rank restarts its pass stamps with the transport
}

int mgicp_comm_attach_shm(mgicp_ctx* ctx, const char* name, size_t max_source_points) {
  if (!ctx) return MGICP_E_INVALID;
  HIPCK(hipSetDevice(ctx->device));
  int rc = cov_join_all(ctx);  // the shard changes under them
  if (rc) return rc;
  rc = reset_stamps(ctx);  // the stamp count restarts with the transport on every rank
  if (rc) return rc;
  if (ctx->have_shm) {
    xgmi_detach(ctx);  // its rendezvous (and the peers' buffers) go with the segment
    (void)hipHostUnregister(ctx->shm.base);
    shm::detach(ctx->shm);
    ctx->have_shm = false;
    ctx->st[kStTransport] = ctx->comm ? 1 : 0;
  }
  if (!name) return MGICP_OK;  // detach only
  if (max_source_points == 0) max_source_points = size_t(32) << 20;
  if (max_source_points >= (size_t(1) << 31))
    return fail(ctx, MGICP_E_INVALID, "max_source_points: at most 2^31 - 2 points per cloud");
  const long long max_sup = static_cast<long long>((max_source_points + kSuperPts - 1) / kSuperPts);
  std::string err;
  shm::Segment seg;
  if (!shm::attach(seg, name, ctx->nranks, ctx->rank, max_sup, ctx->remote_deadline_s, err))
    return fail(ctx, MGICP_E_COMM, err);
  // the GPU writes its rows straight into the segment: map it into the device's address space
  hipError_t e = hipHostRegister(seg.base, seg.bytes, hipHostRegisterMapped);
  void* d = nullptr;
  if (e == hipSuccess) e = hipHostGetDevicePointer(&d, seg.base, 0);
  if (e != hipSuccess) {
    (void)hipHostUnregister(seg.base);
    shm::detach(seg);
    return fail(ctx, MGICP_E_HIP, std::string("hipHostRegister of the shared row segment: ") + hipGetErrorString(e));
  }
  ctx->shm = seg;
  ctx->shm_d = static_cast<unsigned char*>(d);
  ctx->have_shm = true;  // row stamps and gather indices count from the attach (reset_stamps above)
  ctx->st[kStTransport] = ctx->comm ? 3 : 2;
  return MGICP_OK;
}

}  // extern "C"
