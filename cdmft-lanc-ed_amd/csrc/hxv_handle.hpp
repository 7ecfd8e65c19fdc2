// The opaque handle behind include/hxv.h and the error helpers shared by the translation units
// that implement the C-ABI (hxv_capi.hip: handles + products; hxv_lanczos.hip: Lanczos recurrences; hxv_ladder.hip: c / c^dagger between sectors;
// hxv_eigh.hip: thick-restart eigensolver).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "hxv_internal.hpp"
#include "hxv_tiles.hpp"

struct hxv_handle;
namespace hxv {
int fail(int code, const std::string& msg);  // records the message hxv_last_error() returns; returns code
constexpr int RED_BLOCKS = 1024;             // workgroups of the grid-stride reduction kernels
// slots of the Lanczos scalars in device memory: hxv_handle::d_scalars [8]; the paired driver has a block of 2*LZ_PAIR of its own, the second
// component's scalars LZ_PAIR behind the first one's
enum LzSlot : int {
  LZ_ALPHA = 0,
  LZ_BETA = 1,
  LZ_S = 2,        // s = 1/beta_k: the stored vector times s is the unit Lanczos vector
  LZ_C = 3,        // c = beta_k/beta_{k-1}: coefficient of the previous stored vector
  LZ_ALPHA_S = 4,  // alpha*s: coefficient of the stored vector in the subtract-and-norm pass
  LZ_TMP = 5,      // norms and checks outside the recurrence
  LZ_STEP = 6,     // step counter of the device-only iterations (lz_next)
  LZ_AGREE = 7,    // comm_agree's status all-reduce (hxv_transport.cpp)
  LZ_PAIR = 8
};
// vector-sized device buffers go through the engine's cache (hxv_pool.cpp): a fresh hipMalloc costs ~25 ms per GB here
hipError_t pool_alloc(int device, size_t bytes, void** out);
void pool_free(int device, void* ptr);
int64_t pool_live_blocks(int device);        // blocks handed out on the device and not yet returned (get_option "pool_live_blocks")
int ensure_wt(hxv_handle* h);                // (re)allocates the dw-hop scratch of the tiled kernels (hxv_capi.hip)
// the two rank transports of a split sector and the collectives over them (hxv_transport.cpp)
bool comm_ready(const hxv_handle* h);
int comm_allreduce_sum(hxv_handle* h, double* d_buf, size_t count, hipStream_t st);  // no-op without a communicator
int comm_sendrecv_cols(hxv_handle* h, const void* send, const int64_t* send_ptr, void* recv, const int64_t* recv_ptr, size_t col_bytes, hipStream_t st);
int comm_allgather_inplace(hxv_handle* h, void* base, size_t slot_bytes, hipStream_t st);  // rank r's slot at base + r * slot_bytes -> every rank's
int comm_agree(hxv_handle* h, int rc_local);  // collective: non-zero on every rank if any rank passes non-zero (no-op without a communicator)
void comm_release_transport(hxv_handle* h);   // comm_release's first half: the handle leaves its communicator / its group
int need_comm(const hxv_handle* h, const char* who);  // HXV_ERR_STATE ("<who> on a split sector needs the communicator...") for a split sector without one
// slab exchange of a split sector: what the product does with those collectives (hxv_exchange.cpp)
bool comm_in_gather(const hxv_handle* h, const void* p);  // p lies in one of the handle's gather buffers (hxv_slab_home)
// this rank's slab -> d_full, every rank's slab at column slot rank*cmax (the padded all-gather layout, whatever exchange mode h uses)
int comm_allgather_slab(hxv_handle* h, const double2* d_v_local, double2* d_full, hipStream_t st);
// (H v)|slab from this rank's slab: exchange + product; `ep`: optional Lanczos epilogue of pass A (its partial sums are this rank's share)
int apply_slab(hxv_handle* h, const double2* d_v_local, double2* d_hv_local, hipStream_t st, const LzEpilogue* ep = nullptr);
int apply_slab_real(hxv_handle* h, const double* d_v_local, double* d_hv_local, hipStream_t st, const LzEpilogue* ep = nullptr);
void comm_release(hxv_handle* h);
// REAL-vector mode helpers shared by the Lanczos drivers (hxv_capi.hip / hxv_lanczos.hip)
const char* real_mode_blocker(const hxv_handle* h);  // nullptr when real vectors can be used with this handle
bool want_real(const hxv_handle* h);                 // option real_vectors is on and nothing blocks it
int pitch_real_of(const hxv_handle* h);
// layout conversions between complex [DimDw][pitch] and real [DimDw][pitch_real] device vectors (pads written as zero)
void launch_to_real(const hxv_handle* h, const double2* src, double* dst, hipStream_t st);
void launch_to_complex(const hxv_handle* h, const double* src, double2* dst, hipStream_t st);
// scal[slot] of h->d_scalars = |x|^2 (op 0) or |x| (op 1) of the n double2 elements of x, over all ranks of a split sector, enqueued on the
// handle's stream (hxv_lanczos.hip)
int enqueue_norm(hxv_handle* h, const double2* x, int64_t n, int slot, int op);
// THE argument check of a probe list, for the four entries that take one (hxv_lanczos.hip): the range of nprobes, and with nprobes > 0 the list,
// the entry's output arrays (have_outputs; `outputs` names them in the message), every entry of the list, and that no probe lies in a gather
// buffer of the handle (why_gather: what would happen to it there).  HXV_ERR_ARG with "<who>: ..." or HXV_OK.
int check_probe_list(const hxv_handle* h, const char* who, int nprobes, const void* const* d_probes, bool have_outputs, const char* outputs,
                     const char* why_gather);
// deterministic start vector of this rank's slab (a hash of the global reference index) / its real part
void launch_init(const hxv_handle* h, double2* q, uint64_t seed, hipStream_t st);
void launch_init_real(const hxv_handle* h, double* q, uint64_t seed, hipStream_t st);
// split sector: the slab's home in the three gather buffers, for the three Lanczos vectors (HXV_ERR_HIP: no memory for them)
int comm_lz_homes(hxv_handle* h, bool real, double2* out[3]);
// this rank's slab between a HOST array in the reference's layout (contiguous columns of DimUp, the reference's row order) and a DEVICE vector
// (columns padded to pitch, rows in the device row order with the basis signs of SectorHost::up_perm).  Synchronous: returns when the copy is
// done.  The reference's order on the device: one 2-D copy; a device row order: one contiguous copy + one permuting pass through a buffer from
// the engine's cache.
int slab_from_host(hxv_handle* h, const void* v_host, double2* d_vec);
int slab_to_host(hxv_handle* h, const double2* d_vec, void* v_host);
int finish_create(hxv_handle* h, int device, hxv_handle** out);  // builds the tile plan, uploads the tables of h->img (hxv_capi.hip); deletes h on failure

// Device tables of a sector travel in ONE allocation and ONE host-to-device copy: a sector has ~50 of them (maps, ELL tables, tile
// tables of both spins) and a hipMalloc + synchronous hipMemcpy each cost more than building them.  add() copies the table into a
// host staging image at once (the caller's vector may die) and remembers where the device pointer is to be stored; commit() allocates,
// copies and patches the pointers, which must still be alive then.
struct TableArena {
  struct Item {
    size_t off;
    void** dst;
  };
  std::vector<char> stage;
  std::vector<Item> items;
  template <typename T>
  hipError_t add(const std::vector<T>& v, T** p) {
    const size_t off = (stage.size() + 255) & ~(size_t)255, bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
    stage.resize(off + bytes, 0);
    if (!v.empty()) std::memcpy(stage.data() + off, v.data(), v.size() * sizeof(T));
    items.push_back({off, (void**)p});
    *p = nullptr;
    return hipSuccess;
  }
  // -> the base of the allocation (the caller owns it: hipFree), its size in *bytes
  hipError_t commit(void** base, int64_t* bytes) {
    *base = nullptr;
    *bytes = (int64_t)std::max<size_t>(stage.size(), 256);
    hipError_t e = hipMalloc(base, (size_t)*bytes);
    if (e != hipSuccess) return e;
    if (!stage.empty()) e = hipMemcpy(*base, stage.data(), stage.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return e;
    for (const Item& it : items) *it.dst = (char*)*base + it.off;
    items.clear();
    std::vector<char>().swap(stage);
    return hipSuccess;
  }
};

// hipFree of device allocations that belong to `device`, whatever the caller's current device is, which is restored (hxv_cache.cpp).  An
// empty list calls nothing of the HIP runtime.
void free_on_device(int device, const std::vector<void*>& allocs);
inline int compute_units(int device) {  // what the drivers cut their work lists for; 256 where the runtime does not say
  int ncu = 0;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu < 1) ncu = 256;
  return ncu;
}
// Device tables a driver derives from a sector image and keeps with it (TableStore below): `base` is what TableArena::commit returned, `more`
// further allocations of a set that is filled piece by piece.  The destructor frees them on their device.
struct DeviceTables {
  void* base = nullptr;
  std::vector<void*> more;
  int device = -1;
  int64_t bytes = 0;
  DeviceTables() = default;
  DeviceTables(const DeviceTables&) = delete;
  DeviceTables& operator=(const DeviceTables&) = delete;
  virtual ~DeviceTables();
};
// The table sets of one sector image, by driver family ("observables", "spin pair", ...) and key, most recently used last within a family.
// Outside the sector cache's byte budget.  A driver reaches its tables through get() alone; adding a driver adds nothing here.
struct TableStore {
  struct Entry {
    std::string family, key;
    std::shared_ptr<DeviceTables> tables;
  };
  std::mutex mu;
  std::vector<Entry> entries;
  // out = the tables of (family, key): the stored ones, or what build(out) makes now -- a builder that fails (non-zero) stores nothing, the
  // next call builds again --, after which the family keeps its `cap` most recently used sets (a call under way keeps a dropped set alive
  // through its own reference).  Then ensure(*out), for sets that are completed on demand.  All of it under the store's lock: a table set
  // is built once per image.  -> what build or ensure returned.
  template <typename T, typename Build, typename Ensure>
  int get(const char* family, const std::string& key, size_t cap, std::shared_ptr<T>& out, Build build, Ensure ensure) {
    std::lock_guard<std::mutex> lk(mu);
    auto it = std::find_if(entries.begin(), entries.end(), [&](const Entry& e) { return e.family == family && e.key == key; });
    if (it != entries.end()) {
      std::rotate(it, it + 1, entries.end());
    } else {
      std::shared_ptr<T> made;
      if (int rc = build(made)) return rc;
      const auto same = [&](const Entry& e) { return e.family == family; };
      if ((size_t)std::count_if(entries.begin(), entries.end(), same) >= cap) entries.erase(std::find_if(entries.begin(), entries.end(), same));
      entries.push_back({family, key, made});
    }
    out = std::static_pointer_cast<T>(entries.back().tables);
    return ensure(*out);
  }
  template <typename T, typename Build>
  int get(const char* family, const std::string& key, size_t cap, std::shared_ptr<T>& out, Build build) {
    return get(family, key, cap, out, build, [](T&) { return 0; });
  }
};
// What opening a sector builds and never changes afterwards: the host description (basis maps, one-spin matrices, diagonal tables),
// the tile plan of the default options and every device table of both.  Handles SHARE it (shared_ptr): the reference re-opens the
// same sector for every Green's-function channel (build_Hv_sector / delete_Hv_sector around each sp_lanc_tridiag, ED_GF_NORMAL.f90:208-222),
// and the images of closed sectors stay in a per-process cache keyed by everything that determines them (hxv_capi.hip: sector_cache).
struct SectorImage {
  SectorHost host;
  DevSector dev{};
  TilePlan plan;
  int kernel = 1;                 // 0: too many distinct amplitudes for the tile kernels
  int device = -1;
  std::vector<void*> allocs;      // device allocations (the table arena)
  int64_t device_bytes = 0, host_bytes = 0;
  std::string key;                // full cache key (compared byte for byte); empty: not cacheable (from_csr, panels)
  double us_host = 0, us_plan = 0, us_upload = 0;  // what building it cost (microseconds)
  bool uploaded = false;
  // between the host half of an open (tile plan built, every table staged) and its device half (one allocation, one copy): the staged
  // tables and the device pointers they will be patched into
  struct Pending;
  std::shared_ptr<Pending> pending;
  // what the drivers derive from this image on first use: observables, density matrices, density operators, spin pair INTO this sector
  TableStore tables;
  ~SectorImage();
};
// the cache of closed sectors' images (hxv_cache.cpp); an empty key means "do not cache"
std::string sector_cache_key(const hxv_model& m, int nup, int ndw, int rank, int nranks, int device, int exchange);
std::shared_ptr<SectorImage> sector_cache_find(const std::string& key);
void sector_cache_insert(const std::shared_ptr<SectorImage>& im);
// the fused Lanczos step (hxv_lanczos.hip) for callers that keep their own basis (hxv_eigh_lowest); _available: may this handle use the
// fused product at all (the device drivers ask the same question)
bool lanczos_local_step_available(const hxv_handle* h);
int lanczos_local_step(hxv_handle* h, bool real, const double2* q, double sq, const double2* qm, double sqm, double beta, double2* w,
                       bool sub_alpha, double* alpha, double* nrm_w);
// exchange mode 2 on a split sector: pass A reads the dw part in pieces (one block per rank of origin) and runs on the tile kernel
inline bool dw_part_in_pieces(const hxv_handle* h);
}  // namespace hxv

#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess)                                                                              \
      return hxv::fail(HXV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                \
  } while (0)

namespace hxv {
inline std::atomic<int64_t> g_live_handles{0};  // hxv_live_handles(): handles created and not yet destroyed (leak checks of host programs)
}
struct hxv_handle {
  std::shared_ptr<hxv::SectorImage> img;  // shared, immutable (see SectorImage); `host` below is img->host
  hxv::SectorHost& host;
  explicit hxv_handle(std::shared_ptr<hxv::SectorImage> i = std::make_shared<hxv::SectorImage>()) : img(std::move(i)), host(img->host) { ++hxv::g_live_handles; }
  ~hxv_handle() { --hxv::g_live_handles; }
  hxv_handle(const hxv_handle&) = delete;
  hxv_handle& operator=(const hxv_handle&) = delete;
  double open_us[4] = {0, 0, 0, 0};       // this open: host build, tile plan, upload, whole call (get_option "open_us_*"); 0 0 0 on a cache hit
  int open_cache_hit = 0;
  int device = 0;
  hipStream_t stream = nullptr;
  std::vector<void*> allocs;
  hxv::DevSector dev{};
  hxv::TilePlan plan;
  // staging for hxv_apply_host
  double2* d_stage_v = nullptr;
  double2* d_stage_hv = nullptr;
  double2* d_wt = nullptr;  // dw-hop scratch of the tiled kernels (column-group-blocked, tiled_wt_elems())
  int64_t wt_elems = 0;
  // lanczos scratch
  double* d_partials = nullptr;  // [2][RED_BLOCKS]
  double* d_scalars = nullptr;   // [8]
  double2* d_lz[3] = {nullptr, nullptr, nullptr};
  double2* lz_vec[3] = {nullptr, nullptr, nullptr};  // what the drivers use: d_lz[], or (split sector) the slab's home in three gather buffers
  int lz_inplace = 1;              // option "lanczos_inplace": on a split sector the Lanczos vectors live in their slot of a gather buffer (no slab copy per product)
  double* d_lz_partial = nullptr;  // per-workgroup partial sums of the fused Lanczos epilogue
  int64_t lz_partial_n = 0;
  double* h_probe_ov = nullptr;    // page-locked host staging of hxv_lanczos_tridiag_probes: a step's overlaps land here by a truly asynchronous copy
  int64_t probe_ov_n = 0;          // (grown on demand, freed with the handle)
  int lz_fused = 1;                // option "lanczos_fused"
  int lz_graph = 1;                // option "lanczos_graph": fixed-length tridiagonalisations run device-only, three iterations per hipGraph
  int eigh_measure_all = 0;        // option "eigh_measure_all": hxv_eigh_lowest measures every projection at every step (round-1 behaviour)
  int64_t eigh_last_full = 0, eigh_last_local = 0;  // Gram-Schmidt passes of the last hxv_eigh_lowest: whole basis / local only
  int64_t eigh_last_search = 0, eigh_last_check = 0;  // products of the last hxv_eigh_lowest: the search / the check rounds for hidden copies
  // which restart code the last hxv_eigh_lowest ran: thick restarts of the search round, those whose rotation went through launch_rotate_dots,
  // and restart cycles (any round) whose first step went through tr_axpy_mdot
  int64_t eigh_last_restarts = 0, eigh_last_fused_restarts = 0, eigh_last_fused_first = 0;
  int eigh_fuse_restart = 1;       // option "eigh_fuse_restart": the restart rotation measures the residual vector, the first step of a cycle removes the arrow and measures in one pass
  int eigh_keep_pct = 20;          // option "eigh_keep_pct": share of the basis beyond the wanted pairs that a thick restart keeps
  int eigh_degenerate = 0;         // option "eigh_degenerate": 1 = hxv_eigh_lowest looks for further copies of degenerate levels (locking rounds; C3: +60
                                   // products on 380); 0 [default] = one Krylov space, what ARPACK (the call this replaces) does
  int real_vectors = 1;            // option "real_vectors": device Lanczos drivers use real vectors when H and the start vector are real
  int lz_buf_mode = 0;             // layout the d_lz work vectors were last used in (0 complex, 1 real): the pad rows differ
  int last_real = 0;               // did the last device Lanczos run use real vectors (get_option "lanczos_real_last")
  int kernel = 1;
  // split sector: RCCL communicator over the nranks handles (hxv_comm_init) and the gathered vector
  void* comm = nullptr;          // ncclComm_t
  void* comm_shared = nullptr;   // hxv_transport.cpp ProcComm: the PROCESS-level communicator `comm` belongs to (one ncclCommInitRank per process and
                                 // (nranks, rank, device, library), shared by every sector the process opens; ED_VARS_GLOBAL.f90:365-380 sets MpiComm once
                                 // per solve); null: thread ranks / none
  std::atomic<int> comm_aborted{0};  // hxv_comm_abort has run (from ANOTHER host thread while this rank's own sits in a collective) on `comm` (freed by ncclCommAbort: never destroyed again, never used again)
  void* comm_api = nullptr;      // the RCCL entry points that communicator was created with (hxv_transport.cpp: the system's librccl, or HXV_RCCL_LIB)
  void* lgroup = nullptr;        // thread ranks of one process (hxv_comm_init_local): the group object, see hxv_transport.cpp
  double2* d_gather = nullptr;   // nranks * cmax * pitch elements (all-gather layout) / (qdw + halo) * pitch (halo layout)
  double2* d_gather_x[2] = {nullptr, nullptr};  // two more of the same for the device Lanczos on a split sector (three vectors rotate)
  double2* gather_cur = nullptr; // the gather buffer the last exchange ran on (apply_slab reads the gathered vector there)
  int a2a_overlap = 0;           // option "exchange_overlap": exchange mode 2 runs diagonal + up hops on a second stream while the transposes are under way
  hipStream_t stream2 = nullptr; // that second stream and its two events (created on first use)
  hipEvent_t ov_ev[2] = {nullptr, nullptr};
  void* a2a = nullptr;           // exchange 2 (two all-to-all transposes): panel handle, staging buffers, per-peer offsets (hxv_exchange.cpp)
  int64_t n_slab_copy = 0;       // slab copies into a gather buffer (exchange with a vector that is not at home)
  double2* d_send = nullptr;     // halo exchange: packed columns, grouped by destination rank
  int32_t* d_send_cols = nullptr;
  int64_t n_exchange = 0;
  int64_t n_allreduce = 0;       // sum all-reduces of a split sector since creation (comm_allreduce_sum with a communicator; get_option "allreduce_count")
  int64_t n_apply = 0;
  std::vector<void*> owned_vectors;      // hxv_vector_alloc'ed and not yet freed (hxv_destroy returns what is left to the buffer cache)
  int64_t h2d_bytes = 0, d2h_bytes = 0;  // vector-sized PCIe traffic of the host-array entry points and hxv_vector_from/to_host (hxv_get_stats)
  int64_t device_bytes = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t kt_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // hxv_time_apply_slab: events around the kernels of a slab product (two regions in exchange mode 2; [4], [5]: pass A on the second stream of its overlapped form)
  int kt_on = 0;
  hipEvent_t tw_ev[4] = {nullptr, nullptr, nullptr, nullptr};  // split hxv_twin_vector into this handle: before pack / after pack / after the exchange / after unpack (created on first use)
  int64_t twin_last_us[3] = {-1, -1, -1};  // ... and what the three phases of the last such call took on the stream, microseconds (get_option "twin_last_*_us")
  int64_t last_overlapped_us = 0;  // last hxv_time_apply_slab: mean time of the kernels that ran on the second stream beside the exchange (overlapped mode 2), microseconds

  template <typename T>
  hipError_t alloc(T** p, size_t n) {
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    hipError_t e = hipMalloc((void**)p, bytes);
    if (e == hipSuccess) {
      allocs.push_back((void*)*p);
      device_bytes += (int64_t)bytes;
    }
    return e;
  }
  template <typename T>
  hipError_t upload(T** p, const std::vector<T>& src) {
    hipError_t e = alloc(p, src.size());
    if (e != hipSuccess) return e;
    if (!src.empty()) e = hipMemcpy(*p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
  }
};

inline bool hxv::dw_part_in_pieces(const hxv_handle* h) { return h->host.exchange == 2 && h->host.nranks > 1; }

namespace hxv {
// room for `want` doubles in the handle's page-locked staging array h_probe_ov (grown on demand, never shrunk, freed with the handle): where
// the sums of a driver's step land by a truly asynchronous copy
inline int ensure_probe_stage(hxv_handle* h, int64_t want) {
  if (want <= h->probe_ov_n) return HXV_OK;
  if (h->h_probe_ov) (void)hipHostFree(h->h_probe_ov);
  h->h_probe_ov = nullptr;
  h->probe_ov_n = 0;
  HIPCHK(hipHostMalloc((void**)&h->h_probe_ov, (size_t)want * sizeof(double), hipHostMallocDefault));
  h->probe_ov_n = want;
  return HXV_OK;
}
}  // namespace hxv
