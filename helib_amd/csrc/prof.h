// prof.h -- in-situ kernel timing with HIP events (host code only).
//
// Every kernel launch of the library goes through HX_LAUNCH.  Between hx_profile_begin() and
// hx_profile_end() each launch carries a pair of events that take the dispatch's own start and stop
// timestamps (hipExtLaunchKernelGGL: no extra barrier or cache write-back between kernels, which a
// hipEventRecord pair would insert -- measured: it made the mod-down apply kernel look 8 % slower than
// rocprofv3 sees it), so a kernel is timed where it actually runs -- between its real neighbours inside
// a multiply, with their cache and clock state -- and not in a back-to-back loop of its own.
// bench.py derives `roofline` from this (the rocprofv3 kernel trace of the same command, committed
// under profiles/, is the cross-check); outside a profiling window a launch costs one predictable
// branch.  Launches recorded into a HIP graph are skipped (events cannot bracket them).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cxxabi.h>
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

namespace hxp {

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: raise it once per (device, kernel)
// -- a process-wide `static bool` (rounds 1-5) left a second context on another device with the default 64 KiB limit
// (its first large-LDS launch failed) and let two contexts' threads race on the flag.
// The registry is a fixed open-addressed table of atomics keyed on (device, kernel): the steady state -- every launch
// after a kernel's first on a device -- is one probe of two loads, no lock (a mutex and a std::map lookup
// sat on every row-kernel launch).  `device`: the context's own (hx_ctx::device, the current device under CTX_ENTER);
// call sites without a context at hand leave it out and the current device is asked for.
inline hipError_t dyn_lds(const void* kern, int bytes, int device = -1)
{
  struct Slot {
    std::atomic<uintptr_t> key{0};   // kernel address | (device + 1) << 48; 0: free
    std::atomic<int> bytes{0};       // limit granted (published before the key)
  };
  constexpr unsigned SLOTS = 4096;   // (a few hundred kernels x the devices of one box)
  static Slot tab[SLOTS];
  static std::mutex mu;              // taken by the first launch of a kernel on a device only
  if (device < 0) {
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess)
      return e;
  }
  const uintptr_t key = ((uintptr_t)kern & (((uintptr_t)1 << 48) - 1)) | ((uintptr_t)(device + 1) << 48);
  const unsigned h0 = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 52);   // 12 bits
  for (unsigned i = 0, h = h0; i < SLOTS; i++, h = (h + 1) & (SLOTS - 1)) {
    const uintptr_t k = tab[h].key.load(std::memory_order_acquire);
    if (k == key) {
      if (tab[h].bytes.load(std::memory_order_acquire) >= bytes)
        return hipSuccess;
      break;
    }
    if (k == 0)
      break;
  }
  std::lock_guard<std::mutex> lk(mu);
  Slot* s = nullptr;
  for (unsigned i = 0, h = h0; i < SLOTS && !s; i++, h = (h + 1) & (SLOTS - 1)) {
    const uintptr_t k = tab[h].key.load(std::memory_order_relaxed);
    if (k == key || k == 0)
      s = &tab[h];
  }
  if (s && s->key.load(std::memory_order_relaxed) == key && s->bytes.load(std::memory_order_relaxed) >= bytes)
    return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess && s) {   // (a full table: the attribute is set again at every launch, which is still correct)
    s->bytes.store(bytes, std::memory_order_release);
    s->key.store(key, std::memory_order_release);
  }
  return e;
}

struct Rec {
  int name, device;
  unsigned wgs, wg_size;
  hipEvent_t e0, e1;
};
struct State {
  std::mutex mu;
  std::vector<std::string> names;
  std::unordered_map<const void*, int> by_ptr;
  std::vector<Rec> recs;
  std::map<int, std::vector<hipEvent_t>> spare;   // by device: an event is reused on the device it was created on
  size_t dropped = 0;
  std::string summary;                            // of the window that ended last, until it has been fetched
  bool have_summary = false;
};
// read by every launch from any thread, written under State::mu by begin() / end()
inline std::atomic<bool> enabled{false};
inline State& state()
{
  static State s;
  return s;
}
static constexpr size_t MAX_RECS = (size_t)1 << 18;

inline hipEvent_t take_event(State& s, int device)
{
  hipEvent_t e = nullptr;
  std::vector<hipEvent_t>& pool = s.spare[device];
  if (!pool.empty()) {
    e = pool.back();
    pool.pop_back();
  } else if (hipEventCreate(&e) != hipSuccess) {
    (void)hipGetLastError();
    e = nullptr;
  }
  return e;
}

// registers the launch; true: launch with (e0, e1) as the dispatch's start / stop events
inline bool pre(const void* fn, const char* text, hipStream_t st, dim3 grid, dim3 block, hipEvent_t* e0, hipEvent_t* e1)
{
  State& s = state();
  std::lock_guard<std::mutex> lk(s.mu);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (cs != hipStreamCaptureStatusNone)
    return false;
  if (s.recs.size() >= MAX_RECS) {
    s.dropped++;
    return false;
  }
  auto it = s.by_ptr.find(fn);
  if (it == s.by_ptr.end()) {
    // the instantiated kernel's name as rocprofv3 prints it
    std::string nm;
    const char* mangled = hipKernelNameRefByPtr(fn, st);
    if (mangled) {
      int status = 0;
      char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
      nm = (status == 0 && dem) ? dem : mangled;
      free(dem);
    } else {
      (void)hipGetLastError();
      nm = text;
    }
    const size_t paren = nm.find('(');  // drop the argument list
    if (paren != std::string::npos && paren > 0)
      nm.resize(paren);
    if (nm.rfind("void ", 0) == 0)
      nm.erase(0, 5);
    s.names.push_back(nm);
    it = s.by_ptr.emplace(fn, (int)s.names.size() - 1).first;
  }
  Rec r;
  r.name = it->second;
  r.device = 0;
  if (hipGetDevice(&r.device) != hipSuccess)
    (void)hipGetLastError();
  r.wgs = grid.x * grid.y * grid.z;
  r.wg_size = block.x * block.y * block.z;
  r.e0 = take_event(s, r.device);
  r.e1 = take_event(s, r.device);
  if (!r.e0 || !r.e1) {
    if (r.e0)
      s.spare[r.device].push_back(r.e0);
    if (r.e1)
      s.spare[r.device].push_back(r.e1);
    s.dropped++;
    return false;
  }
  s.recs.push_back(r);
  *e0 = r.e0;
  *e1 = r.e1;
  return true;
}

inline int begin()
{
  State& s = state();
  std::lock_guard<std::mutex> lk(s.mu);
  for (Rec& r : s.recs) {
    s.spare[r.device].push_back(r.e0);
    s.spare[r.device].push_back(r.e1);
  }
  s.recs.clear();
  s.dropped = 0;
  s.summary.clear();
  s.have_summary = false;
  enabled.store(true, std::memory_order_relaxed);
  return 0;
}
// waits for the recorded launches; JSON: {"launches": n, "dropped": d, "kernels": [{"kernel", "workgroups",
// "workgroup_size", "calls", "total_us", "avg_us", "min_us", "max_us"} ... by total time]}
// The window closes at the FIRST call (recording stops there whatever becomes of the summary); the summary is kept
// -- under the mutex, for whichever thread asks -- until fetch = true hands it out or the next begin() drops it.
inline std::string end(bool fetch)
{
  State& s = state();
  std::lock_guard<std::mutex> lk(s.mu);
  enabled.store(false, std::memory_order_relaxed);
  if (s.have_summary) {
    std::string out = s.summary;
    if (fetch) {
      s.summary.clear();
      s.have_summary = false;
    }
    return out;
  }
  struct Agg {
    size_t calls = 0;
    double total = 0, mn = 1e30, mx = 0;
    unsigned wg_size = 0;
  };
  std::map<std::pair<int, unsigned>, Agg> agg;
  size_t bad = 0;
  for (Rec& r : s.recs) {
    float ms = 0;
    if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) {
      (void)hipGetLastError();
      bad++;
    } else {
      Agg& a = agg[{r.name, r.wgs}];
      const double us = (double)ms * 1e3;
      a.calls++;
      a.total += us;
      a.mn = us < a.mn ? us : a.mn;
      a.mx = us > a.mx ? us : a.mx;
      a.wg_size = r.wg_size;
    }
    s.spare[r.device].push_back(r.e0);
    s.spare[r.device].push_back(r.e1);
  }
  const size_t n = s.recs.size();
  s.recs.clear();
  std::vector<std::pair<double, std::pair<int, unsigned>>> order;
  for (auto& kv : agg)
    order.push_back({-kv.second.total, kv.first});
  std::sort(order.begin(), order.end());
  std::string out = "{\"launches\": " + std::to_string(n) + ", \"dropped\": " + std::to_string(s.dropped + bad) +
                    ", \"kernels\": [";
  bool first = true;
  for (auto& o : order) {
    const Agg& a = agg[o.second];
    std::string nm;
    for (char ch : s.names[(size_t)o.second.first])
      if (ch != '"' && ch != '\\')
        nm.push_back(ch);
    char buf[256];
    snprintf(buf, sizeof buf,
             "\"workgroups\": %u, \"workgroup_size\": %u, \"calls\": %zu, \"total_us\": %.2f, \"avg_us\": %.3f, "
             "\"min_us\": %.3f, \"max_us\": %.3f}",
             o.second.second, a.wg_size, a.calls, a.total, a.total / (double)a.calls, a.mn, a.mx);
    out += std::string(first ? "" : ", ") + "{\"kernel\": \"" + nm + "\", " + buf;
    first = false;
  }
  out += "]}";
  if (!fetch) {
    s.summary = out;
    s.have_summary = true;
  }
  return out;
}

}  // namespace hxp

#define HX_LAUNCH(kern, grid, block, lds, st, ...)                                                        \
  do {                                                                                                     \
    const dim3 _hx_g = (grid), _hx_b = (block);                                                            \
    hipEvent_t _hx_e0, _hx_e1;                                                                             \
    if (hxp::enabled.load(std::memory_order_relaxed) && hxp::pre((const void*)(kern), #kern, (st), _hx_g, _hx_b, &_hx_e0, &_hx_e1))        \
      hipExtLaunchKernelGGL(kern, _hx_g, _hx_b, (lds), (st), _hx_e0, _hx_e1, 0, __VA_ARGS__);              \
    else                                                                                                   \
      hipLaunchKernelGGL(kern, _hx_g, _hx_b, (lds), (st), __VA_ARGS__);                                    \
  } while (0)
