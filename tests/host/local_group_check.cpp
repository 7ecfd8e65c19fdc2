// TEST-ONLY: the host logic of a rank group run alone (csrc/hxv_local_group.hpp, nothing else of the project): no HIP, no device, no handle.
// Driven by tests/test_host_local_group_check.py: plain, under -fsanitize=address,undefined and under -fsanitize=thread.
//
//   local_group_check MODE     MODE = barrier | timeout | abort | agree | sum | cache; the thread ranks are std::threads, 2, 3, 4 and 8 of them.
// Last line of stdout: "LOCAL_GROUP_CHECK mode=<mode> checks=<n> failures=<n> OK|FAILED"; every failure is a line "FAIL ..." on stderr.
#include <atomic>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <thread>

#include "hxv_local_group.hpp"

using namespace hxv;
using Clock = std::chrono::steady_clock;

static std::atomic<long> g_checks{0}, g_failures{0};
#define CHECK(cond, ...)                        \
  do {                                          \
    ++g_checks;                                 \
    if (!(cond)) {                              \
      ++g_failures;                             \
      std::fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);        \
      std::fprintf(stderr, "\n");               \
    }                                           \
  } while (0)

static const int SIZES[] = {2, 3, 4, 8};
static double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }
// `count` threads, each running body(rank)
static void run_ranks(int count, const std::function<void(int)>& body) {
  std::vector<std::thread> th;
  for (int r = 0; r < count; ++r) th.emplace_back(body, r);
  for (auto& t : th) t.join();
}

// 2000 generations: nobody leaves generation g before all n have entered it
static void mode_barrier() {
  for (int n : SIZES) {
    RankGroup G(n);
    std::atomic<long> entered{0};
    std::atomic<long> early{0}, failed{0};
    run_ranks(n, [&](int) {
      for (long g = 0; g < 2000; ++g) {
        ++entered;
        if (G.barrier()) ++failed;
        if (entered.load() < (g + 1) * n) ++early;
      }
    });
    CHECK(failed == 0, "n=%d: %ld barriers returned non-zero", n, failed.load());
    CHECK(early == 0, "n=%d: %ld returns before every rank had entered", n, early.load());
    CHECK(entered == 2000L * n && G.gen == 2000 && G.arrived == 0 && !G.broken, "n=%d: gen %llu arrived %d", n, (unsigned long long)G.gen, G.arrived);
  }
}

// n-1 ranks arrive, one never does: all return non-zero in bounded time, and every later call fails at once
static void mode_timeout() {
  for (int n : SIZES) {
    RankGroup G(n);
    G.timeout_s = 0.2;
    run_ranks(n - 1, [&](int r) {
      const auto t0 = Clock::now();
      const int rc = G.barrier();
      const double dt = seconds_since(t0);
      CHECK(rc != 0, "n=%d rank %d: the barrier without its last rank returned 0", n, r);
      CHECK(dt < 5.0, "n=%d rank %d: returned after %.3f s", n, r, dt);
      for (int k = 0; k < 3; ++k) {
        const auto t1 = Clock::now();
        const int rc2 = G.barrier();
        const double dt2 = seconds_since(t1);
        CHECK(rc2 != 0 && dt2 < 0.1, "n=%d rank %d: later call %d returned %d after %.3f s", n, r, k, rc2, dt2);
      }
    });
    CHECK(G.broken, "n=%d: the group is not marked broken", n);
  }
}

// a thread that is no rank aborts while n-1 ranks wait (default timeout: 300 s): all wake with non-zero
static void mode_abort() {
  for (int n : SIZES) {
    RankGroup G(n);
    const auto t0 = Clock::now();
    std::thread foreign([&] {
      for (;;) {
        {
          std::lock_guard<std::mutex> lk(G.mu);
          if (G.arrived == n - 1) break;
        }
        std::this_thread::yield();
      }
      G.abort();
      G.abort();  // (any number of times)
    });
    run_ranks(n - 1, [&](int r) {
      const int rc = G.barrier();
      CHECK(rc != 0, "n=%d rank %d: woke with 0 after the abort", n, r);
      CHECK(G.barrier() != 0, "n=%d rank %d: a barrier after the abort returned 0", n, r);
    });
    foreign.join();
    CHECK(seconds_since(t0) < 30.0, "n=%d: the abort took %.1f s to wake the ranks", n, seconds_since(t0));
  }
}

// the result is the rank's own non-zero status, else the first non-zero in rank order
static void agree_case(int n, const std::vector<int>& status, bool broken) {
  RankGroup G(n);
  if (broken) G.abort();
  int first = 0;
  for (int p = n - 1; p >= 0; --p)
    if (status[p]) first = status[p];
  run_ranks(n, [&](int r) {
    for (int round = 0; round < (broken ? 1 : 20); ++round) {  // (back to back: the second barrier protects the flags of the next round)
      bool broke = !broken;
      const int mine = status[r] && !broken ? status[r] + 100 * (round % 2) : status[r];
      const int got = G.agree(r, mine, &broke);
      const int want = broken || mine || !first ? mine : first + 100 * (round % 2);
      CHECK(got == want && broke == broken, "n=%d rank %d: agree -> %d (broke %d), expected %d (broke %d)", n, r, got, (int)broke, want, (int)broken);
    }
  });
}
static void mode_agree() {
  for (int n : SIZES) {
    agree_case(n, std::vector<int>(n, 0), false);
    for (int k = 0; k < n; ++k) {
      std::vector<int> s(n, 0);
      s[k] = 5 + k;
      agree_case(n, s, false);  // one rank non-zero: it gets its own value, the others the same
      agree_case(n, s, true);   // broken group: everybody gets its own status back
    }
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < n; ++b) {
        if (a == b) continue;
        std::vector<int> s(n, 0);
        s[a] = 7;
        s[b] = -9;  // (a < b and a > b: rank order decides, not the value)
        agree_case(n, s, false);
      }
  }
}

// every rank's total has the bits of the left-to-right sum over ranks 0..n-1 from 0.0, which the check computes itself
static void mode_sum() {
  const double vals[4] = {1e16, 1.0, -1e16, 3.0};
  const size_t COUNT = 6;  // elements 0-3: the four values dealt to the ranks at four shifts; 4: -0.0 from everybody; 5: rank and round
  for (int n : SIZES) {
    RankGroup G(n);
    const int shorter = n - 1;  // this rank contributes two elements fewer
    auto contribution = [&](int p, int round) {
      std::vector<double> v(p == shorter ? COUNT - 2 : COUNT);
      for (size_t i = 0; i < v.size(); ++i) v[i] = i < 4 ? vals[(p + i) % 4] * (1 + round % 3) : i == 4 ? -0.0 : 0.1 * (p + 1) + round;
      return v;
    };
    std::atomic<long> wrong{0}, failed{0};
    run_ranks(n, [&](int r) {
      for (int round = 0; round < 500; ++round) {
        const std::vector<double> mine = contribution(r, round);
        std::vector<double> tot(mine.size(), -1.0), want(mine.size(), 0.0);
        if (G.sum(r, mine, tot.data())) ++failed;
        for (int p = 0; p < n; ++p) {
          const std::vector<double> c = contribution(p, round);
          for (size_t i = 0; i < want.size() && i < c.size(); ++i) want[i] += c[i];
        }
        if (std::memcmp(tot.data(), want.data(), want.size() * sizeof(double)) != 0) ++wrong;
      }
    });
    CHECK(failed == 0 && wrong == 0, "n=%d: %ld sums failed, %ld differ in their bits from the rank-ordered sum", n, failed.load(), wrong.load());
    // the order does matter for these contributions, and -0.0 alone sums to +0.0 from the 0.0 the sum starts at
    std::vector<double> rev(COUNT, 0.0), fwd(COUNT, 0.0);
    for (int p = 0; p < n; ++p)
      for (size_t i = 0; i < contribution(p, 0).size(); ++i) fwd[i] += contribution(p, 0)[i];
    for (int p = n - 1; p >= 0; --p)
      for (size_t i = 0; i < contribution(p, 0).size(); ++i) rev[i] += contribution(p, 0)[i];
    if (n >= 4) CHECK(std::memcmp(fwd.data(), rev.data(), 4 * sizeof(double)) != 0, "n=%d: the contributions sum alike in either order", n);
    CHECK(fwd[4] == 0.0 && !std::signbit(fwd[4]), "n=%d: -0.0 only", n);
  }
  RankGroup B(2);
  B.abort();
  double t = 0.0;
  CHECK(B.sum(0, {1.0}, &t) != 0, "sum on a broken group returned 0");
}

// ---- the communicator cache's bookkeeping ---------------------------------------------------------------------------------------------------
struct Entry : CachedComm {
  int key = 0, id = 0;
  std::atomic<int> destroyed{0}, bound{0}, bound_at_destroy{0};
};
static void destroy_entry(CachedComm* c) {
  Entry* e = static_cast<Entry*>(c);
  if (e->bound.load() != 0) ++e->bound_at_destroy;
  ++e->destroyed;  // (kept alive: the check reads the counts at the end)
}

static void cache_threads() {
  CommBook book(destroy_entry);
  std::mutex reg_mu;
  std::vector<std::unique_ptr<Entry>> reg;
  std::atomic<long> binds{0}, seen_destroyed{0};
  run_ranks(8, [&](int t) {
    std::mt19937 rng(1000 + t);
    for (int round = 0; round < 3000; ++round) {
      const int key = (int)(rng() % 12);
      Entry* e = static_cast<Entry*>(book.bind([&](CachedComm* c) { return static_cast<Entry*>(c)->key == key; }));
      if (!e) {
        e = new Entry();
        e->key = key;
        book.insert(e, rng() % 8 != 0);  // (one in eight belongs to its maker alone, like HXV_COMM_CACHE=0)
        std::lock_guard<std::mutex> lk(reg_mu);
        reg.emplace_back(e);
      }
      ++binds;
      ++e->bound;
      if (rng() % 16 == 0) book.evict(e);
      if (rng() % 8 == 0) (void)book.clear();
      if (e->destroyed.load() != 0) ++seen_destroyed;
      --e->bound;
      book.release(e);
    }
  });
  (void)book.clear();
  long once = 0, while_bound = 0;
  for (auto& e : reg) {
    once += e->destroyed == 1;
    while_bound += e->bound_at_destroy.load();
  }
  CHECK(once == (long)reg.size(), "threads: %ld of %zu entries destroyed exactly once", once, reg.size());
  CHECK(while_bound == 0 && seen_destroyed == 0, "threads: %ld destroyed while bound, %ld seen destroyed by a user", while_bound, seen_destroyed.load());
  CHECK(book.inits + book.reuses == binds && book.inits == (int64_t)reg.size(), "threads: inits %lld + reuses %lld, binds %ld", (long long)book.inits,
        (long long)book.reuses, binds.load());
  CHECK(book.all.empty(), "threads: %zu entries left after the last clear", book.all.size());
}

// one thread, a seeded walk of binds, releases, evictions and clears against the same policy written down again
static void cache_script() {
  CommBook book(destroy_entry);
  std::vector<std::unique_ptr<Entry>> reg;
  struct Model { int key, users; bool listed, destroyed; };
  std::vector<Model> model;     // by id
  std::vector<int> order;       // ids of the listed entries, oldest first
  std::vector<int> held;        // ids of the references the script holds (an id may repeat)
  int64_t inits = 0, reuses = 0;
  std::mt19937 rng(7);
  for (int step = 0; step < 4000; ++step) {
    const unsigned op = rng() % 10;
    if (op < 5) {  // bind, or make
      const int key = (int)(rng() % 12);
      int want = -1;
      for (int id : order)
        if (want < 0 && model[id].key == key) want = id;
      Entry* e = static_cast<Entry*>(book.bind([&](CachedComm* c) { return static_cast<Entry*>(c)->key == key; }));
      CHECK((e ? e->id : -1) == want, "script step %d: bind found %d, the policy says %d", step, e ? e->id : -1, want);
      if (e) {
        ++model[want].users;
        ++reuses;
      } else {
        const bool list = rng() % 6 != 0;
        e = new Entry();
        e->key = key;
        e->id = (int)reg.size();
        reg.emplace_back(e);
        book.insert(e, list);
        model.push_back({key, 1, list, false});
        if (list) order.push_back(e->id);
        ++inits;
      }
      held.push_back(e->id);
    } else if (op < 8 && !held.empty()) {  // release one reference: the last user of an entry that is not listed destroys it
      const size_t k = rng() % held.size();
      const int id = held[k];
      held.erase(held.begin() + (long)k);
      book.release(reg[id].get());
      if (--model[id].users == 0 && !model[id].listed) model[id].destroyed = true;
    } else if (op == 8 && !held.empty()) {  // evict an entry the script holds: no later bind finds it
      const int id = held[rng() % held.size()];
      book.evict(reg[id].get());
      model[id].listed = false;
      order.erase(std::remove(order.begin(), order.end(), id), order.end());
    } else if (op == 9) {  // clear: the listed entries without a user go
      int64_t want = 0;
      std::vector<int> keep;
      for (int id : order) {
        if (model[id].users == 0) {
          model[id].listed = false;
          model[id].destroyed = true;
          ++want;
        } else {
          keep.push_back(id);
        }
      }
      order.swap(keep);
      const int64_t got = book.clear();
      CHECK(got == want, "script step %d: clear destroyed %lld, the policy says %lld", step, (long long)got, (long long)want);
    }
    bool same = book.all.size() == order.size() && book.inits == inits && book.reuses == reuses;
    for (size_t i = 0; same && i < order.size(); ++i) same = static_cast<Entry*>(book.all[i])->id == order[i];
    for (size_t id = 0; same && id < model.size(); ++id)
      same = reg[id]->destroyed == (model[id].destroyed ? 1 : 0) && reg[id]->users == model[id].users && reg[id]->listed == model[id].listed;
    CHECK(same, "script step %d: the cache's state differs from the policy's", step);
  }
  CHECK(inits > 20 && reuses > 500, "script: %lld inits, %lld reuses", (long long)inits, (long long)reuses);
}
static void mode_cache() {
  cache_threads();
  cache_script();
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "barrier") mode_barrier();
  else if (mode == "timeout") mode_timeout();
  else if (mode == "abort") mode_abort();
  else if (mode == "agree") mode_agree();
  else if (mode == "sum") mode_sum();
  else if (mode == "cache") mode_cache();
  else {
    std::fprintf(stderr, "usage: local_group_check barrier|timeout|abort|agree|sum|cache\n");
    return 2;
  }
  std::printf("LOCAL_GROUP_CHECK mode=%s checks=%ld failures=%ld %s\n", mode.c_str(), g_checks.load(), g_failures.load(), g_failures ? "FAILED" : "OK");
  return g_failures ? 1 : 0;
}
