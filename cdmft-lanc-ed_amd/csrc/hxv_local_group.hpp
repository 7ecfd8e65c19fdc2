// The host logic of a rank group (hxv_transport.cpp): the barrier of the thread ranks with its timeout and abort, their status agreement,
// their rank-ordered sum, what each rank offers to the collective under way, and the bookkeeping of the process-wide communicator cache.
// Host C++ only: no HIP, no handle, no RCCL type.  The header lives apart so that tests/host/local_group_check.cpp can compile it with a
// plain host compiler, under the address, undefined-behaviour and thread sanitizers.
#pragma once

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <vector>

namespace hxv {

// What a rank offers to the pull under way: peers read it between the collective's two barriers, never the rank's handle.
struct RankOffer {
  const char* base = nullptr;    // device buffer the peers copy from
  const int64_t* ptr = nullptr;  // per-destination offsets into it (column exchange), or null
};

// ---- thread ranks: the ranks of a sector are host threads of this process -----------------------------------------
struct RankGroup {
  int n = 0;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  uint64_t gen = 0;
  std::vector<std::vector<double>> red;  // by rank: contribution to the running all-reduce
  std::vector<int> flag;                 // by rank: agree()
  std::vector<RankOffer> offer;          // by rank: the collective under way
  bool broken = false;                   // a rank dropped out (abort()) or a barrier timed out: every wait returns an error
  double timeout_s = 300.0;              // HXV_LOCAL_TIMEOUT_S
  explicit RankGroup(int nranks) : n(nranks), red(nranks), flag(nranks, 0), offer(nranks) {}
  // Every rank calls it; returns 0 when all have (the ranks issue their collectives in the same order, like MPI ranks), non-zero when the
  // group is broken: a peer was aborted, or did not arrive in time (then this rank breaks the group for everybody else).
  int barrier() {
    std::unique_lock<std::mutex> lk(mu);
    if (broken) return 1;
    const uint64_t g = gen;
    if (++arrived == n) {
      arrived = 0;
      ++gen;
      cv.notify_all();
      return 0;
    }
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::duration<double>(timeout_s);
    while (gen == g && !broken)
      if (cv.wait_until(lk, deadline) == std::cv_status::timeout && gen == g) {
        broken = true;
        cv.notify_all();
      }
    return gen == g ? 1 : 0;
  }
  // wakes every rank that waits in a barrier and makes every later one fail; callable from any thread, any number of times
  void abort() {
    std::lock_guard<std::mutex> lk(mu);
    broken = true;
    cv.notify_all();
  }
  // Status agreement: the rank's own non-zero status, else the first non-zero in rank order, else 0.  A barrier that breaks sets
  // *broke and returns the rank's own status.
  int agree(int rank, int rc_local, bool* broke) {
    int worst = rc_local;
    flag[rank] = rc_local;
    if ((*broke = barrier() != 0)) return rc_local;
    for (int p = 0; p < n; ++p)
      if (flag[p] != 0 && worst == 0) worst = flag[p];
    if ((*broke = barrier() != 0)) return rc_local;
    return worst;
  }
  // tot[i] = sum over the ranks, in rank order on every rank (the same bits everywhere), of what each deposited; non-zero: group broken
  int sum(int rank, const std::vector<double>& mine, double* tot) {
    const size_t count = mine.size();
    red[rank] = mine;
    if (barrier()) return 1;
    std::fill(tot, tot + count, 0.0);
    for (int p = 0; p < n; ++p)
      for (size_t i = 0; i < count && i < red[p].size(); ++i) tot[i] += red[p][i];
    return barrier();  // (everybody has read every contribution before anybody overwrites its own)
  }
};

// ---- the communicator cache's bookkeeping: which entries can be found, who is bound to them, who destroys them ------------------
struct CachedComm {
  int users = 0;        // handles bound to it   } both guarded by CommBook::mu
  bool listed = false;  // bind() can find it    }
};
// An entry is destroyed exactly once and never while a user holds it: by release() of its last user when it is not (or no longer)
// listed, by clear() when it is listed and idle.  Both decide under mu.
struct CommBook {
  std::mutex mu;
  std::vector<CachedComm*> all;   // the listed entries
  int64_t inits = 0, reuses = 0;  // entries made / binds served by an entry that existed already
  void (*const destroy)(CachedComm*);
  explicit CommBook(void (*d)(CachedComm*)) : destroy(d) {}
  template <class Match>
  CachedComm* bind(Match&& match) {
    std::lock_guard<std::mutex> lk(mu);
    for (CachedComm* e : all)
      if (match(e)) {
        ++e->users;
        ++reuses;
        return e;
      }
    return nullptr;
  }
  // a new entry, bound to its maker; `list`: later binds may find it (else it belongs to that one user)
  void insert(CachedComm* e, bool list) {
    std::lock_guard<std::mutex> lk(mu);
    ++inits;
    e->users = 1;
    e->listed = list;
    if (list) all.push_back(e);
  }
  void release(CachedComm* e) {
    std::unique_lock<std::mutex> lk(mu);
    if (--e->users != 0 || e->listed) return;
    lk.unlock();
    destroy(e);
  }
  // the entry serves no further bind (it failed, or was aborted); its users keep it until they release it.  The caller is one of them.
  void evict(CachedComm* e) {
    std::lock_guard<std::mutex> lk(mu);
    all.erase(std::remove(all.begin(), all.end(), e), all.end());
    e->listed = false;
  }
  // destroys every listed entry nobody is bound to; -> how many
  int64_t clear() {
    std::vector<CachedComm*> gone;
    {
      std::lock_guard<std::mutex> lk(mu);
      std::vector<CachedComm*> keep;
      for (CachedComm* e : all) (e->users == 0 ? gone : keep).push_back(e);
      all.swap(keep);
      for (CachedComm* e : gone) e->listed = false;
    }
    for (CachedComm* e : gone) destroy(e);
    return (int64_t)gone.size();
  }
};

}  // namespace hxv
