// The two rank transports behind the slab exchange of the C-ABI (hxv_exchange.cpp): one communicator per open (split) sector, and the
// collectives over it.  Nothing here knows a vector layout or launches a kernel; a collective never reads a peer's handle.
// Two transports serve the same code path:
//   * RCCL over xGMI, one process per GPU: hxv_comm_unique_id (rank 0) -> broadcast the 128 bytes with the host program's
//     own MPI_Bcast -> hxv_comm_init on every rank.  RCCL is loaded with dlopen at the first of these calls: the library has
//     no link-time dependency on it, and a process that already holds a copy (PyTorch ships its own) reuses it.
//   * THREAD RANKS inside one process: hxv_comm_local_create(nranks) -> hxv_comm_init_local(handle, group) from one host
//     thread per rank.  Slabs travel by device-to-device copies ordered with HIP events, scalars through host memory.  The
//     ranks may share one GPU (how the multi-rank code paths -- uneven slabs, halo lists, the drivers' collectives --
//     are executed and tested on a one-GPU box, where RCCL refuses two ranks on one device) or sit on different GPUs of
//     a node driven by one process.
// The dot products of the device Lanczos drivers are all-reduced on the same stream (comm_allreduce_sum), and a rank that
// fails before a collective tells the others first (comm_agree), so that nobody waits for a peer that has already left.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cstdlib>
#include <map>

#include "hxv_handle.hpp"
#include "hxv_local_group.hpp"

using namespace hxv;

namespace {
struct Rccl {
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclCommAbort) CommAbort = nullptr;  // optional: hxv_comm_abort
  std::string path;                              // file the symbols came from (dladdr)
  std::string err;
};
// One symbol table per library.  HXV_RCCL_LIB (read at every hxv_comm_unique_id / hxv_comm_init) names the library to use instead of the
// system's librccl: the test suite points it at tests/rccl_double (thread ranks of ONE process behind RCCL's ten entry points), which is
// how the RCCL branches below execute with several ranks on a one-GPU box.  A communicator keeps the table it was created with
// (hxv_handle::comm_api), so handles of both kinds can live in one process.
Rccl* rccl() {
  static std::mutex mu;
  static std::map<std::string, std::unique_ptr<Rccl>> tables;
  const char* over = getenv("HXV_RCCL_LIB");
  const std::string key = over && over[0] ? over : "";
  std::lock_guard<std::mutex> lk(mu);
  auto it = tables.find(key);
  if (it != tables.end()) return it->second.get();
  std::unique_ptr<Rccl> t(new Rccl());
  Rccl& r = *t;
  if (!key.empty()) {
    r.lib = dlopen(key.c_str(), RTLD_NOW | RTLD_LOCAL);
  } else {
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.lib) break;
    }
  }
  if (!r.lib) {
    const char* de = dlerror();
    r.err = std::string("cannot load ") + (key.empty() ? "librccl" : key) + ": " + (de ? de : "?");
  } else {
#define SYM(field, sym)                                           \
  r.field = reinterpret_cast<decltype(r.field)>(dlsym(r.lib, #sym)); \
  if (!r.field) r.err = "the RCCL library lacks " #sym;
    SYM(GetUniqueId, ncclGetUniqueId)
    SYM(CommInitRank, ncclCommInitRank)
    SYM(CommDestroy, ncclCommDestroy)
    SYM(AllGather, ncclAllGather)
    SYM(AllReduce, ncclAllReduce)
    SYM(GetErrorString, ncclGetErrorString)
    SYM(Send, ncclSend)
    SYM(Recv, ncclRecv)
    SYM(GroupStart, ncclGroupStart)
    SYM(GroupEnd, ncclGroupEnd)
#undef SYM
    r.CommAbort = reinterpret_cast<decltype(r.CommAbort)>(dlsym(r.lib, "ncclCommAbort"));  // (not required of a library)
    {
      // where the library was found: the first real N>1 run must be able to say WHICH librccl it ran (bench.py: config.rccl_lib)
      Dl_info di;
      if (r.GetUniqueId && dladdr(reinterpret_cast<void*>(r.GetUniqueId), &di) && di.dli_fname) r.path = di.dli_fname;
    }
  }
  return tables.emplace(key, std::move(t)).first->second.get();
}
Rccl* api(const hxv_handle* h) { return static_cast<Rccl*>(h->comm_api); }
int nccl_fail(const Rccl* r, const char* what, ncclResult_t e) {
  return fail(HXV_ERR_HIP, std::string(what) + ": " + (r && r->GetErrorString ? r->GetErrorString(e) : "RCCL error"));
}

// ---- ONE communicator per process, not per sector ---------------------------------------------------------
// The reference sets MpiComm once per solve (ED_VARS_GLOBAL.f90:365-380, ed_set_MpiComm) and derives a sub-communicator only for sectors with
// DimDw < MpiSize (ED_HAMILTONIAN.f90:63-89); its callers open 289 sectors per ED_DIAG sweep (ED_DIAG.f90:142-190) and 56 per Green's-function
// stage (ED_GF_NORMAL.f90:208-222).  ncclCommInitRank is a collective that builds rings and channels over xGMI -- hundreds of milliseconds on a
// node -- so the engine builds it ONCE per (library, nranks, rank, device) and every later hxv_comm_init with the same key binds the handle to
// that communicator (the id it is given is then not consumed: all ranks take the same branch, because all ranks have made the same calls).
// A sector with DimDw < nranks is opened by the first DimDw ranks with nranks' = DimDw: another key, built once as well.
// HXV_COMM_CACHE=0: one communicator per handle, as before round 6.  An aborted communicator leaves the cache.
// The cache's bookkeeping (who is bound, who destroys, inits / reuses) is the CommBook of hxv_local_group.hpp: users and listed of the base.
struct ProcComm : CachedComm {
  ncclComm_t c = nullptr;
  Rccl* api = nullptr;
  int nranks = 0, rank = 0, device = 0;
  std::atomic<int> aborted{0};
  std::atomic<int> failed{0};     // a collective on it returned an error: torn down with ncclCommAbort (ncclCommDestroy may wait for the lost peer)
};
ProcComm* pc(const hxv_handle* h) { return static_cast<ProcComm*>(h->comm_shared); }
void proc_comm_destroy(CachedComm* e) {
  ProcComm* p = static_cast<ProcComm*>(e);
  (void)hipSetDevice(p->device);
  if (p->c && !p->aborted) {  // (ncclCommAbort has freed an aborted communicator)
    if (p->failed && p->api->CommAbort)
      (void)p->api->CommAbort(p->c);
    else
      (void)p->api->CommDestroy(p->c);
  }
  delete p;
}
CommBook& comm_cache() {
  static CommBook c(proc_comm_destroy);
  return c;
}
bool comm_cache_on() {
  const char* e = getenv("HXV_COMM_CACHE");
  return !(e && e[0] == '0');
}
// A collective on the handle's communicator has FAILED (a peer aborted, a link went down): the communicator must not serve the next sector.
// It leaves the cache (the next hxv_comm_init builds a new one from its id); the handles bound to it keep it until they are closed.
int comm_failed(hxv_handle* h, const char* what, ncclResult_t e) {
  if (ProcComm* p = pc(h)) {
    p->failed = 1;
    comm_cache().evict(p);
  }
  return nccl_fail(api(h), what, e);
}

// ---- thread ranks: the host logic is the RankGroup of hxv_local_group.hpp; here its HIP events and who has joined ---------------
struct LocalGroup : RankGroup {
  std::vector<hxv_handle*> member;      // by rank: join, leave and destroy only; no collective reads a peer's handle
  std::vector<hipEvent_t> ready, done;  // by rank: "what I offer is in place" / "I have read what the others offer"
  explicit LocalGroup(int nranks) : RankGroup(nranks), member(nranks, nullptr), ready(nranks, nullptr), done(nranks, nullptr) {}
};
int broken_group() { return fail(HXV_ERR_STATE, "thread-rank group: a peer rank dropped out (aborted, failed or did not arrive in time); the group is unusable"); }
// a HIP call inside a collective of the thread-rank transport: the error is remembered, the rank still takes part in the collective's
// barriers (its peers must not be left waiting) and reports after the last one
#define HIPREC(expr)                                                                                        \
  do {                                                                                                      \
    hipError_t _e = (expr);                                                                                 \
    if (_e != hipSuccess && rc == HXV_OK) rc = fail(HXV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)
LocalGroup* lg(const hxv_handle* h) { return reinterpret_cast<LocalGroup*>(h->lgroup); }

// THE pull of the thread-rank transport, two barriers: every rank publishes its offer and records `ready`; after the first barrier it waits
// for each peer's `ready` and enqueues the copy that plan(p, peer's offer) asks for (bytes == 0: none); it records `done`, and after the
// second barrier waits for every peer's `done` -- what it offered is free again once they have read it.
struct PullCopy {
  void* dst = nullptr;
  const void* src = nullptr;
  size_t bytes = 0;
};
template <class Plan>
int local_pull(LocalGroup* G, int rank, RankOffer mine, hipStream_t st, Plan&& plan) {
  int rc = HXV_OK;
  G->offer[rank] = mine;
  HIPREC(hipEventRecord(G->ready[rank], st));
  if (G->barrier()) return broken_group();
  for (int p = 0; p < G->n; ++p) {
    if (p == rank) continue;
    const PullCopy c = plan(p, G->offer[p]);
    if (!c.bytes || rc) continue;
    HIPREC(hipStreamWaitEvent(st, G->ready[p], 0));
    HIPREC(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDefault, st));
  }
  HIPREC(hipEventRecord(G->done[rank], st));
  if (G->barrier()) return broken_group();
  for (int p = 0; p < G->n; ++p)
    if (p != rank) HIPREC(hipStreamWaitEvent(st, G->done[p], 0));
  return rc;
}
}  // namespace

namespace hxv {
// Columns of `cb` bytes between the ranks of h's communicator: rank r sends send[send_ptr[p] .. send_ptr[p+1]) to every peer p and
// receives recv[recv_ptr[p] .. recv_ptr[p+1]) from it (offsets in columns; both buffers on the device; asynchronous on st).  The
// halo exchange of the product and the column moves of the spin-dw ladder operators are this one step.
int comm_sendrecv_cols(hxv_handle* h, const void* send_v, const int64_t* send_ptr, void* recv_v, const int64_t* recv_ptr, size_t cb, hipStream_t st) {
  const SectorHost& s = h->host;
  const char* send = reinterpret_cast<const char*>(send_v);
  char* recv = reinterpret_cast<char*>(recv_v);
  if (LocalGroup* G = lg(h)) {
    int bad = 0;
    const int rc = local_pull(G, s.rank, RankOffer{send, send_ptr}, st, [&](int p, const RankOffer& o) {
      const size_t nr = (size_t)(recv_ptr[p + 1] - recv_ptr[p]);
      if ((size_t)(o.ptr[s.rank + 1] - o.ptr[s.rank]) != nr) bad = 1;  // the two ranks' plans disagree
      if (!nr || bad) return PullCopy{};
      return PullCopy{recv + (size_t)recv_ptr[p] * cb, o.base + (size_t)o.ptr[s.rank] * cb, nr * cb};
    });
    if (rc) return rc;
    if (bad) return fail(HXV_ERR_STATE, "column exchange: a peer's send list does not match this rank's receive list");
    return HXV_OK;
  }
  if (!h->comm) return fail(HXV_ERR_STATE, "column exchange without a communicator");
  Rccl* r = api(h);
  ncclResult_t e = r->GroupStart();
  for (int p = 0; p < s.nranks && e == ncclSuccess; ++p) {
    if (p == s.rank) continue;
    const size_t ns = (size_t)(send_ptr[p + 1] - send_ptr[p]) * cb / sizeof(double), nr = (size_t)(recv_ptr[p + 1] - recv_ptr[p]) * cb / sizeof(double);
    if (ns) e = r->Send(send + (size_t)send_ptr[p] * cb, ns, ncclFloat64, p, (ncclComm_t)h->comm, st);
    if (nr && e == ncclSuccess) e = r->Recv(recv + (size_t)recv_ptr[p] * cb, nr, ncclFloat64, p, (ncclComm_t)h->comm, st);
  }
  ncclResult_t e2 = r->GroupEnd();
  if (e != ncclSuccess || e2 != ncclSuccess) return comm_failed(h, "grouped send/recv", e != ncclSuccess ? e : e2);
  return HXV_OK;
}

// In-place all-gather of equal slots: rank r's slot_bytes at base + r * slot_bytes reach the same place of every rank's buffer.
int comm_allgather_inplace(hxv_handle* h, void* base_v, size_t slot_bytes, hipStream_t st) {
  char* base = reinterpret_cast<char*>(base_v);
  if (LocalGroup* G = lg(h))
    return local_pull(G, h->host.rank, RankOffer{base, nullptr}, st,
                      [&](int p, const RankOffer& o) { return PullCopy{base + (size_t)p * slot_bytes, o.base + (size_t)p * slot_bytes, slot_bytes}; });
  if (!h->comm) return fail(HXV_ERR_STATE, "whole-vector gather without a communicator");
  ncclResult_t e = api(h)->AllGather(base + (size_t)h->host.rank * slot_bytes, base, slot_bytes / sizeof(double), ncclFloat64, (ncclComm_t)h->comm, st);
  if (e != ncclSuccess) return comm_failed(h, "ncclAllGather", e);
  return HXV_OK;
}

bool comm_ready(const hxv_handle* h) {
  const bool gone = h->comm_aborted || (h->comm_shared && static_cast<const ProcComm*>(h->comm_shared)->aborted);
  return (h->comm != nullptr && !gone) || h->lgroup != nullptr;
}

int comm_allreduce_sum(hxv_handle* h, double* d_buf, size_t count, hipStream_t st) {
  if (comm_ready(h)) ++h->n_allreduce;
  if (LocalGroup* G = lg(h)) {
    // through host memory, summed in rank order on every rank: the same bits everywhere
    int rc = HXV_OK;
    std::vector<double> mine(count, 0.0), tot(count, 0.0);
    HIPREC(hipMemcpyAsync(mine.data(), d_buf, count * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPREC(hipStreamSynchronize(st));
    if (G->sum(h->host.rank, mine, tot.data())) return broken_group();
    HIPREC(hipMemcpyAsync(d_buf, tot.data(), count * sizeof(double), hipMemcpyHostToDevice, st));
    HIPREC(hipStreamSynchronize(st));
    return rc;
  }
  if (!h->comm) return HXV_OK;  // serial: nothing to add
  ncclResult_t e = api(h)->AllReduce(d_buf, d_buf, count, ncclFloat64, ncclSum, (ncclComm_t)h->comm, st);
  if (e != ncclSuccess) return comm_failed(h, "ncclAllReduce", e);
  return HXV_OK;
}

// Collective error agreement: every rank passes its local status; all return non-zero if any rank failed.  Called by the
// drivers after their rank-local preparations (allocations, argument checks) and BEFORE their first collective, so that a
// rank that cannot go on does not leave its peers waiting inside an all-reduce.
int comm_agree(hxv_handle* h, int rc_local) {
  if (!comm_ready(h)) return rc_local;
  int worst = rc_local;
  if (LocalGroup* G = lg(h)) {
    bool broke = false;
    worst = G->agree(h->host.rank, rc_local, &broke);
    if (broke) return rc_local ? rc_local : broken_group();
  } else {
    double v = rc_local ? 1.0 : 0.0;
    hipError_t e = hipMemcpyAsync(h->d_scalars + LZ_AGREE, &v, sizeof(double), hipMemcpyHostToDevice, h->stream);
    ncclResult_t ne = ncclSuccess;
    if (e == hipSuccess) ne = api(h)->AllReduce(h->d_scalars + LZ_AGREE, h->d_scalars + LZ_AGREE, 1, ncclFloat64, ncclMax, (ncclComm_t)h->comm, h->stream);
    if (e == hipSuccess && ne == ncclSuccess) e = hipMemcpyAsync(&v, h->d_scalars + LZ_AGREE, sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess && ne == ncclSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess || ne != ncclSuccess) return fail(HXV_ERR_HIP, "comm_agree: the status all-reduce failed");
    if (v != 0.0 && worst == 0) worst = HXV_ERR_STATE;
  }
  if (worst != 0 && rc_local == 0) return fail(worst, "a peer rank of this sector reported an error before the collective step: all ranks stop");
  return worst;
}

// comm_release's transport half: the handle leaves its communicator or its group
void comm_release_transport(hxv_handle* h) {
  if (h->comm) {
    // the communicator belongs to the process (cache) or to this handle alone (HXV_COMM_CACHE=0 / taken out of the cache by an abort)
    if (ProcComm* p = pc(h)) comm_cache().release(p);
    h->comm = nullptr;
    h->comm_shared = nullptr;
    h->comm_api = nullptr;
    h->comm_aborted = 0;
  }
  if (LocalGroup* G = lg(h)) {
    // (the group object itself belongs to whoever created it: hxv_comm_local_destroy)
    std::lock_guard<std::mutex> lk(G->mu);
    if (h->host.rank < (int)G->member.size() && G->member[h->host.rank] == h) G->member[h->host.rank] = nullptr;
    h->lgroup = nullptr;
  }
}
}  // namespace hxv

extern "C" {

int hxv_comm_unique_id(void* id128) {
  if (!id128) return fail(HXV_ERR_ARG, "hxv_comm_unique_id: NULL");
  Rccl* r = rccl();
  if (!r->err.empty()) return fail(HXV_ERR_UNSUPPORTED, r->err);
  ncclUniqueId id;
  ncclResult_t e = r->GetUniqueId(&id);
  if (e != ncclSuccess) return nccl_fail(r, "ncclGetUniqueId", e);
  static_assert(sizeof(id) == HXV_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
  std::memcpy(id128, &id, sizeof(id));
  return HXV_OK;
}

int hxv_comm_init(hxv_handle* h, const void* id128) {
  if (!h || !id128) return fail(HXV_ERR_ARG, "hxv_comm_init: NULL");
  if (comm_ready(h)) return fail(HXV_ERR_STATE, "hxv_comm_init: the handle already has a communicator");
  if (h->host.panel_rows > 0) return fail(HXV_ERR_STATE, "hxv_comm_init: panel handles take no communicator");
  Rccl* r = rccl();
  if (!r->err.empty()) return fail(HXV_ERR_UNSUPPORTED, r->err);
  HIPCHK(hipSetDevice(h->device));
  const bool use_cache = comm_cache_on();
  ProcComm* p = nullptr;
  if (use_cache)
    p = static_cast<ProcComm*>(comm_cache().bind([&](CachedComm* e) {
      const ProcComm* q = static_cast<const ProcComm*>(e);
      return q->api == r && q->nranks == h->host.nranks && q->rank == h->host.rank && q->device == h->device && !q->aborted;
    }));
  if (!p) {
    ncclUniqueId id;
    std::memcpy(&id, id128, sizeof(id));
    ncclComm_t c = nullptr;
    ncclResult_t e = r->CommInitRank(&c, h->host.nranks, id, h->host.rank);
    if (e != ncclSuccess) return nccl_fail(r, "ncclCommInitRank", e);
    p = new ProcComm();
    p->c = c;
    p->api = r;
    p->nranks = h->host.nranks;
    p->rank = h->host.rank;
    p->device = h->device;
    comm_cache().insert(p, use_cache);
  }
  h->comm = p->c;
  h->comm_shared = p;
  h->comm_api = r;
  return HXV_OK;
}

// The cached communicators of this process (see ProcComm): *entries alive, *inits = ncclCommInitRank calls made since the process started,
// *reuses = hxv_comm_init calls that bound a handle to a communicator that existed already.  Any out may be NULL.
int hxv_comm_cache_stats(int64_t* entries, int64_t* inits, int64_t* reuses) {
  CommBook& cc = comm_cache();
  std::lock_guard<std::mutex> lk(cc.mu);
  if (entries) *entries = (int64_t)cc.all.size();
  if (inits) *inits = cc.inits;
  if (reuses) *reuses = cc.reuses;
  return HXV_OK;
}

// ncclCommDestroy of every cached communicator no handle is bound to (collective in the RCCL sense: every rank of a communicator calls it at the
// same point of the program -- the end of a solve); communicators still in use stay.  Returns the number destroyed through *destroyed.
int hxv_comm_cache_clear(int64_t* destroyed) {
  const int64_t gone = comm_cache().clear();
  if (destroyed) *destroyed = gone;
  return HXV_OK;
}

int hxv_comm_local_create(int32_t nranks, void** group) {
  if (nranks < 1 || !group) return fail(HXV_ERR_ARG, "hxv_comm_local_create: bad argument");
  LocalGroup* G = new LocalGroup(nranks);
  if (const char* t = getenv("HXV_LOCAL_TIMEOUT_S")) {
    const double v = atof(t);
    if (v > 0.0) G->timeout_s = v;
  }
  *group = G;
  return HXV_OK;
}

// A rank of the group cannot go on (its host thread failed outside the library): wake every peer that waits in a collective and make
// every later collective of the group return HXV_ERR_STATE.  Callable from any thread, any number of times.
int hxv_comm_local_abort(void* group) {
  LocalGroup* G = reinterpret_cast<LocalGroup*>(group);
  if (!G) return fail(HXV_ERR_ARG, "hxv_comm_local_abort: NULL");
  G->abort();
  return HXV_OK;
}

// A rank of the communicator has failed OUTSIDE the library: wake this handle's collectives instead of leaving them waiting for it.
// RCCL: ncclCommAbort (callable from another host thread while this rank's thread sits in a collective; the communicator is gone
// afterwards -- later calls on the handle report a missing communicator, hxv_comm_free / hxv_destroy still clean up).  Thread ranks:
// the whole group is marked broken, like hxv_comm_local_abort.
int hxv_comm_abort(hxv_handle* h) {
  if (!h) return HXV_OK;
  if (LocalGroup* G = lg(h)) {
    G->abort();
    return HXV_OK;
  }
  // (not to be raced with hxv_destroy / hxv_comm_free of the SAME handle: the caller joins or serialises -- hxv/engine.py takes a per-sector
  //  lock around both; the handle's fields are read once, up front)
  void* const comm = h->comm;
  ProcComm* const p = pc(h);
  Rccl* const r = api(h);
  if (!comm || h->comm_aborted || (p && p->aborted)) return HXV_OK;
  if (!r || !r->CommAbort) return fail(HXV_ERR_UNSUPPORTED, "hxv_comm_abort: the RCCL library in use exports no ncclCommAbort");
  h->comm_aborted = 1;
  if (p) {
    // the communicator is shared by every sector of this process: all of them lose it, and the cache forgets it (the next hxv_comm_init
    // builds a new one from the id it is given -- every rank's, because an aborted communicator fails its collectives on every rank)
    if (p->aborted.exchange(1)) return HXV_OK;
    comm_cache().evict(p);
  }
  ncclResult_t e = r->CommAbort((ncclComm_t)comm);
  if (e != ncclSuccess) return nccl_fail(r, "ncclCommAbort", e);
  return HXV_OK;
}

// the file the RCCL entry points of this handle's communicator were resolved from ("" without one): what bench.py reports as config.rccl_lib
const char* hxv_comm_library(const hxv_handle* h) {
  if (!h || !h->comm_api) return "";
  return static_cast<const Rccl*>(h->comm_api)->path.c_str();
}

int hxv_comm_local_destroy(void* group) {
  LocalGroup* G = reinterpret_cast<LocalGroup*>(group);
  if (!G) return HXV_OK;
  for (auto* m : G->member)
    if (m) return fail(HXV_ERR_STATE, "hxv_comm_local_destroy: a handle still belongs to the group (hxv_comm_free / hxv_destroy it first)");
  for (auto* events : {&G->ready, &G->done})
    for (hipEvent_t e : *events)
      if (e) (void)hipEventDestroy(e);
  delete G;
  return HXV_OK;
}

int hxv_comm_init_local(hxv_handle* h, void* group) {
  LocalGroup* G = reinterpret_cast<LocalGroup*>(group);
  if (!h || !G) return fail(HXV_ERR_ARG, "hxv_comm_init_local: NULL");
  if (comm_ready(h)) return fail(HXV_ERR_STATE, "hxv_comm_init_local: the handle already has a communicator");
  if (h->host.panel_rows > 0) return fail(HXV_ERR_STATE, "hxv_comm_init_local: panel handles take no communicator");
  if (h->host.nranks != G->n) return fail(HXV_ERR_ARG, "hxv_comm_init_local: the group's size is not the handle's nranks");
  HIPCHK(hipSetDevice(h->device));
  const int r = h->host.rank;
  {
    std::lock_guard<std::mutex> lk(G->mu);
    if (G->member[r]) return fail(HXV_ERR_STATE, "hxv_comm_init_local: this rank has already joined the group");
    G->member[r] = h;
  }
  if (!G->ready[r]) HIPCHK(hipEventCreateWithFlags(&G->ready[r], hipEventDisableTiming));
  if (!G->done[r]) HIPCHK(hipEventCreateWithFlags(&G->done[r], hipEventDisableTiming));
  h->lgroup = G;
  if (G->barrier()) return broken_group();  // collective: every rank has joined (one host thread per rank)
  return HXV_OK;
}

int hxv_comm_free(hxv_handle* h) {
  if (!h) return HXV_OK;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  comm_release(h);
  return HXV_OK;
}

}  // extern "C"
