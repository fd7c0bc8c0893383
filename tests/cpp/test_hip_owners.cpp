// The owners of HIP events and streams (csrc/hip_buffer.h: BasicEvent, BasicStream, BasicEventPair) over a recording fake in
// place of the runtime, with no device.  Stand-alone host program, built with -fsanitize=address,undefined by
// tests/test_hip_owners_host.py; it uses no HIP function, so it links without the HIP runtime.  usage: test_hip_owners
//
// The fake hands out distinct tokens, keeps for each when it was created, synchronised and destroyed, and fails the n-th
// create when told to.  Checked, for the event owner and the stream owner alike unless named:
//   * empty by default; ensure creates with the given flags (defaults: hipEventDefault, hipStreamNonBlocking); a second
//     ensure creates nothing and keeps the handle; get, operator bool and the conversion to the raw handle agree;
//   * a failed create returns the failing status, leaves the owner empty and destroys nothing; the next ensure creates;
//   * reset destroys once and empties; reset of an empty owner does nothing;
//   * move construction and move assignment hand the handle over, the source is empty, an overwritten handle is destroyed
//     exactly once; self-move assignment keeps the handle;
//   * a stream is synchronised exactly once, before its destroy; an event never;
//   * EventPair::ensure with the second create failing: `begin` is destroyed once at scope end; within the scope a later
//     ensure completes the pair without creating `begin` again;
//   * a std::vector of a struct of owners balances under resize (growth reallocates: the elements move), reassignment of an
//     element to a default-constructed value (a group's Member) and clear;
//   * a timed launch's pair reused after it was moved into the pending list (begin_timed / end_timed) gets new events;
//   * the drain_events pattern: a vector of pairs moved into a local, an early return from the loop over it -- the source is
//     empty, every token destroyed once;
//   * at exit: no token live, none destroyed twice, nothing destroyed or synchronised that was never created.
#include "../../myrrix-recommender_amd/csrc/hip_buffer.h"

#include <cstdint>
#include <cstdio>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

static int failures = 0, checks = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    ++checks;                                             \
    if (!(cond)) {                                        \
      if (++failures <= 20) {                             \
        std::fprintf(stderr, "FAIL %s: ", #cond);         \
        std::fprintf(stderr, __VA_ARGS__);                \
        std::fprintf(stderr, "\n");                       \
      }                                                   \
    }                                                     \
  } while (0)

namespace {

struct Ledger {
  struct Rec {
    bool stream = false;
    unsigned flags = 0;
    int destroys = 0, syncs = 0;
    long sync_at = -1, destroy_at = -1;   // positions in the order of all calls
  };
  std::map<uintptr_t, Rec> rec;
  uintptr_t next = 0x1000;
  long seq = 0;
  int creates = 0;     // successful ones
  int fail_in = 0;     // n > 0: the n-th create from now fails (once)
  int stray = 0;       // a destroy or a synchronise of a token that was never created

  hipError_t create(uintptr_t* out, bool stream, unsigned flags) {
    ++seq;
    if (fail_in > 0 && --fail_in == 0) return hipErrorOutOfMemory;
    *out = next;
    next += 0x10;
    Rec r;
    r.stream = stream;
    r.flags = flags;
    rec[*out] = r;
    ++creates;
    return hipSuccess;
  }
  void synchronize(uintptr_t t) {
    ++seq;
    auto it = rec.find(t);
    if (it == rec.end()) {
      ++stray;
      return;
    }
    it->second.syncs += 1;
    it->second.sync_at = seq;
  }
  void destroy(uintptr_t t) {
    ++seq;
    auto it = rec.find(t);
    if (it == rec.end()) {
      ++stray;
      return;
    }
    it->second.destroys += 1;
    it->second.destroy_at = seq;
  }
  int live() const {
    int n = 0;
    for (const auto& kv : rec) n += kv.second.destroys == 0;
    return n;
  }
  int destroyed() const {
    int n = 0;
    for (const auto& kv : rec) n += kv.second.destroys > 0;
    return n;
  }
  int destroyed_twice() const {
    int n = 0;
    for (const auto& kv : rec) n += kv.second.destroys > 1;
    return n;
  }
  // every destroyed stream: one synchronise, before the destroy; every event: none
  int sync_rule_broken() const {
    int n = 0;
    for (const auto& kv : rec) {
      const Rec& r = kv.second;
      if (!r.stream) n += r.syncs != 0;
      else if (r.destroys) n += !(r.syncs == 1 && r.sync_at < r.destroy_at);
      else n += r.syncs != 0;   // (the owners synchronise only on the way to a destroy)
    }
    return n;
  }
};

Ledger L;

struct FakeEventApi {
  static hipError_t create(hipEvent_t* e, unsigned flags) {
    uintptr_t t = 0;
    const hipError_t rc = L.create(&t, false, flags);
    if (rc == hipSuccess) *e = reinterpret_cast<hipEvent_t>(t);
    return rc;
  }
  static void destroy(hipEvent_t e) { L.destroy(reinterpret_cast<uintptr_t>(e)); }
};
struct FakeStreamApi {
  static hipError_t create(hipStream_t* s, unsigned flags) {
    uintptr_t t = 0;
    const hipError_t rc = L.create(&t, true, flags);
    if (rc == hipSuccess) *s = reinterpret_cast<hipStream_t>(t);
    return rc;
  }
  static void synchronize(hipStream_t s) { L.synchronize(reinterpret_cast<uintptr_t>(s)); }
  static void destroy(hipStream_t s) { L.destroy(reinterpret_cast<uintptr_t>(s)); }
};

using FEvent = mals::BasicEvent<FakeEventApi>;
using FStream = mals::BasicStream<FakeStreamApi>;
using FPair = mals::BasicEventPair<FakeEventApi>;

template <class Owner>
uintptr_t token(const Owner& o) {
  return reinterpret_cast<uintptr_t>(o.get());
}

static_assert(!std::is_copy_constructible<FEvent>::value && !std::is_copy_assignable<FEvent>::value, "move-only");
static_assert(!std::is_copy_constructible<FStream>::value && !std::is_copy_assignable<FStream>::value, "move-only");
static_assert(std::is_nothrow_move_constructible<FEvent>::value && std::is_nothrow_move_assignable<FEvent>::value, "nothrow move");
static_assert(std::is_nothrow_move_constructible<FStream>::value && std::is_nothrow_move_assignable<FStream>::value, "nothrow move");
static_assert(std::is_nothrow_move_constructible<FPair>::value && std::is_nothrow_move_assignable<FPair>::value, "nothrow move");
static_assert(!std::is_copy_constructible<FPair>::value, "move-only");

template <class Owner, class Raw>
void test_owner(const char* what, unsigned default_flags, unsigned other_flags) {
  const int c0 = L.creates, d0 = L.destroyed();
  {
    Owner a;
    CHECK(!a && a.get() == nullptr && static_cast<Raw>(a) == nullptr, "%s: a new owner is empty", what);
    a.reset();
    CHECK(L.creates == c0 && L.destroyed() == d0 && L.stray == 0, "%s: reset of an empty owner does nothing", what);
    CHECK(a.ensure() == hipSuccess && a && L.creates == c0 + 1, "%s: ensure creates", what);
    const uintptr_t t = token(a);
    CHECK(L.rec[t].flags == default_flags, "%s: default flags %u", what, L.rec[t].flags);
    const Raw raw = a;   // what a HIP call that takes the owner receives
    CHECK(raw == a.get() && raw != nullptr, "%s: the conversion gives the handle", what);
    CHECK(a.ensure(other_flags) == hipSuccess && token(a) == t && L.creates == c0 + 1, "%s: a second ensure creates nothing", what);
    CHECK(L.rec[t].flags == default_flags, "%s: the first flags stay", what);
    a.reset();
    CHECK(!a && L.rec[t].destroys == 1, "%s: reset destroys once", what);
    a.reset();
    CHECK(L.rec[t].destroys == 1, "%s: a second reset destroys nothing", what);
    CHECK(a.ensure(other_flags) == hipSuccess && token(a) != t && L.rec[token(a)].flags == other_flags, "%s: ensure after reset, given flags", what);
  }
  CHECK(L.creates == c0 + 2 && L.destroyed() == d0 + 2, "%s: the destructor destroys", what);

  {  // a failed create
    const int c1 = L.creates, d1 = L.destroyed();
    Owner a;
    L.fail_in = 1;
    CHECK(a.ensure() == hipErrorOutOfMemory, "%s: the failing status is returned", what);
    CHECK(!a && a.get() == nullptr && L.creates == c1, "%s: a failed create leaves the owner empty", what);
    a.reset();
    CHECK(L.destroyed() == d1 && L.stray == 0, "%s: ... and destroys nothing", what);
    CHECK(a.ensure() == hipSuccess && a && L.creates == c1 + 1, "%s: the next ensure creates", what);
  }

  {  // moves
    Owner a, b;
    CHECK(a.ensure() == hipSuccess && b.ensure() == hipSuccess, "%s: two owners", what);
    const uintptr_t ta = token(a), tb = token(b);
    CHECK(ta != tb, "%s: distinct tokens", what);
    Owner c(std::move(a));
    CHECK(!a && token(c) == ta && L.rec[ta].destroys == 0, "%s: move construction hands the handle over", what);
    b = std::move(c);
    CHECK(!c && token(b) == ta && L.rec[tb].destroys == 1 && L.rec[ta].destroys == 0, "%s: move assignment destroys the overwritten handle once", what);
    Owner* self = &b;   // (through a pointer: no self-move warning)
    b = std::move(*self);
    CHECK(token(b) == ta && L.rec[ta].destroys == 0, "%s: self-move assignment keeps the handle", what);
    b = Owner();
    CHECK(!b && L.rec[ta].destroys == 1, "%s: assignment of an empty owner destroys", what);
  }
  CHECK(L.live() == 0 && L.destroyed_twice() == 0 && L.sync_rule_broken() == 0, "%s: balanced (%d live, %d twice, %d sync)", what, L.live(),
        L.destroyed_twice(), L.sync_rule_broken());
}

void test_stream_sync_order() {
  uintptr_t t1, t2;
  {
    FStream s;
    CHECK(s.ensure() == hipSuccess, "stream");
    t1 = token(s);
    s.reset();
    CHECK(L.rec[t1].syncs == 1 && L.rec[t1].destroys == 1 && L.rec[t1].sync_at < L.rec[t1].destroy_at, "reset: one synchronise, then the destroy");
    CHECK(s.ensure() == hipSuccess, "stream again");
    t2 = token(s);
    CHECK(L.rec[t2].syncs == 0, "no synchronise while the stream lives");
  }
  CHECK(L.rec[t2].syncs == 1 && L.rec[t2].destroys == 1 && L.rec[t2].sync_at < L.rec[t2].destroy_at, "destructor: one synchronise, then the destroy");
  CHECK(L.rec[t1].syncs == 1 && L.rec[t1].destroys == 1, "the first stream was not touched again");
}

void test_event_pair() {
  uintptr_t tb = 0;
  {
    FPair p;
    CHECK(!p.begin && !p.end, "a new pair is empty");
    const int c0 = L.creates;
    L.fail_in = 2;
    CHECK(p.ensure() == hipErrorOutOfMemory, "the second create fails");
    CHECK(p.begin && !p.end && L.creates == c0 + 1, "begin exists, end does not");
    tb = token(p.begin);
  }
  CHECK(L.rec[tb].destroys == 1, "the half-built pair's begin is destroyed once at scope end");
  {
    FPair p;
    const int c0 = L.creates;
    L.fail_in = 2;
    CHECK(p.ensure() == hipErrorOutOfMemory, "the second create fails");
    tb = token(p.begin);
    CHECK(p.ensure() == hipSuccess && p.begin && p.end, "a later ensure completes the pair");
    CHECK(token(p.begin) == tb && L.creates == c0 + 2 && L.rec[tb].destroys == 0, "begin is not created again");
    CHECK(p.ensure() == hipSuccess && L.creates == c0 + 2, "a complete pair creates nothing");
    FPair q(std::move(p));
    CHECK(!p.begin && !p.end && token(q.begin) == tb && q.end, "a pair moves as a whole");
  }
  CHECK(L.live() == 0 && L.destroyed_twice() == 0, "pairs balanced");
}

// a group's Member: streams, events, plain fields
struct Holder {
  int id = 0;
  FStream compute, comm;
  FEvent solved, exchanged;
  hipError_t init() {
    hipError_t e = compute.ensure();
    if (e == hipSuccess) e = comm.ensure();
    if (e == hipSuccess) e = solved.ensure(hipEventDisableTiming);
    if (e == hipSuccess) e = exchanged.ensure(hipEventDisableTiming);
    return e;
  }
};

void test_vector_of_holders() {
  const int c0 = L.creates, d0 = L.destroyed();
  {
    std::vector<Holder> m;
    m.resize(3);
    for (Holder& h : m) CHECK(h.init() == hipSuccess, "init");
    CHECK(L.creates == c0 + 12 && L.destroyed() == d0, "three holders, twelve tokens");
    const uintptr_t t0 = token(m[0].compute), t2 = token(m[2].exchanged);
    m.resize(40);   // reallocates: the elements move
    CHECK(L.destroyed() == d0 && token(m[0].compute) == t0 && token(m[2].exchanged) == t2, "growth moves the handles, destroys none");
    CHECK(!m[3].compute && !m[39].solved, "new elements are empty");
    const uintptr_t t1[4] = {token(m[1].compute), token(m[1].comm), token(m[1].solved), token(m[1].exchanged)};
    m[1] = Holder();   // what destroy_member ends with
    for (uintptr_t t : t1) CHECK(L.rec[t].destroys == 1, "reassignment destroys the element's token once");
    CHECK(L.destroyed() == d0 + 4 && !m[1].compute && !m[1].exchanged, "... and only those");
    m[1] = Holder();
    CHECK(L.destroyed() == d0 + 4, "reassignment of an empty element destroys nothing");
    // init failing midway (the third create): what was built goes with the element
    L.fail_in = 3;
    CHECK(m[5].init() == hipErrorOutOfMemory && m[5].compute && m[5].comm && !m[5].solved, "a half-built holder");
    m.resize(2);   // shrinks: elements 2 .. 39 go, the half-built one among them
    CHECK(L.destroyed() == d0 + 4 + 4 + 2, "shrinking destroys the elements cut off");
    m.clear();
    CHECK(L.destroyed() == d0 + 14 && L.creates == c0 + 14, "clear destroys the rest");
  }
  CHECK(L.live() == 0 && L.destroyed_twice() == 0 && L.sync_rule_broken() == 0, "holders balanced");
}

// the timed launches of the solver: a pair per launch, moved into the handle's list, the list drained later
struct Pending {
  FPair ev;
  int kind = 0;
  double bytes = 0.0;
};

hipError_t begin_timed(Pending& pe, int kind) {
  pe.kind = kind;
  return pe.ev.ensure();
}
void end_timed(std::vector<Pending>& pending, Pending& pe) { pending.push_back(std::move(pe)); }

// returns how many entries it accounted for; stop_at: the entry at which a runtime call "fails" (-1: none)
int drain(std::vector<Pending>& src, int stop_at) {
  const std::vector<Pending> pending = std::move(src);
  src.clear();
  int done = 0;
  for (const Pending& pe : pending) {
    if (done == stop_at) return done;   // (HIPCHK returning)
    CHECK(pe.ev.begin && pe.ev.end, "a pending entry holds its pair");
    ++done;
  }
  return done;
}

void test_pending_list() {
  for (int stop_at : {-1, 0, 3, 6}) {
    const int c0 = L.creates, d0 = L.destroyed();
    std::vector<Pending> pending;
    {
      Pending pe;   // one local for several launches, as the dual lists' launcher has it
      for (int i = 0; i < 7; ++i) {
        CHECK(begin_timed(pe, i) == hipSuccess && pe.ev.begin && pe.ev.end, "a launch's pair");
        end_timed(pending, pe);
        CHECK(!pe.ev.begin && !pe.ev.end, "the pair left the local");
      }
      // a launch that fails between begin and end: its pair goes with the local
      CHECK(begin_timed(pe, 7) == hipSuccess, "the eighth launch's pair");
    }
    CHECK(L.creates == c0 + 16 && L.destroyed() == d0 + 2 && pending.size() == 7, "seven pairs pending, the eighth destroyed");
    bool distinct = true;
    for (size_t i = 0; i < pending.size(); ++i)
      for (size_t j = 0; j < pending.size(); ++j)
        distinct = distinct && token(pending[i].ev.begin) != token(pending[j].ev.end) && (i == j || token(pending[i].ev.begin) != token(pending[j].ev.begin));
    CHECK(distinct, "every launch has its own events");
    const int done = drain(pending, stop_at);
    CHECK(done == (stop_at < 0 ? 7 : stop_at), "drain stopped at %d", done);
    CHECK(pending.empty(), "the source is empty on whichever path drain returned");
    CHECK(L.destroyed() == d0 + 16 && L.destroyed_twice() == 0, "every token destroyed once (%d of 16)", L.destroyed() - d0);
    CHECK(drain(pending, -1) == 0 && L.destroyed() == d0 + 16, "a second drain finds nothing");
  }
  {  // a list that is not drained goes with its holder (a handle destroyed with timed launches pending)
    const int d0 = L.destroyed();
    {
      std::vector<Pending> pending;
      Pending pe;
      for (int i = 0; i < 3; ++i) {
        CHECK(begin_timed(pe, i) == hipSuccess, "pair");
        end_timed(pending, pe);
      }
    }
    CHECK(L.destroyed() == d0 + 6, "the undrained list's events are destroyed with it");
  }
  CHECK(L.live() == 0 && L.destroyed_twice() == 0, "pending lists balanced");
}

}  // namespace

int main() {
  test_owner<FEvent, hipEvent_t>("event", hipEventDefault, hipEventDisableTiming);
  test_owner<FStream, hipStream_t>("stream", hipStreamNonBlocking, hipStreamDefault);
  test_stream_sync_order();
  test_event_pair();
  test_vector_of_holders();
  test_pending_list();
  CHECK(L.live() == 0, "%d tokens live at exit", L.live());
  CHECK(L.destroyed_twice() == 0, "%d tokens destroyed twice", L.destroyed_twice());
  CHECK(L.stray == 0, "%d destroys or synchronises of tokens never created", L.stray);
  CHECK(L.sync_rule_broken() == 0, "%d tokens break the synchronise rule", L.sync_rule_broken());
  CHECK(L.creates > 50 &&L.destroyed() == L.creates, "%d created, %d destroyed", L.creates, L.destroyed());
  std::printf("checks %d failures %d\n", checks, failures);
  return failures ? 1 : 0;
}
