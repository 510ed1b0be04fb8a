// gather_map.h -- the thread-to-work map of bgv_gf_gather_map_kernel (bgv_gf_linalg.hip) as pure functions: no HIP types,
// so tests/cpp/gather_map_test.cpp compiles them for the host and checks that every (unit, j < d) is owned exactly once
// and that no other lane stores (work_map.h is the model).
//
// A unit is one (descriptor, slot) pair: d words in, d words out.  It is held by a group of dp = the next power of two
// >= d lanes (1 .. 64), lane j of the group owning word j, so a wave64 holds 64 / dp units and a workgroup of 256 threads
// 256 / dp.  The launch has `blocks` workgroups and runs `passes` passes, the same number for every thread -- the kernel
// shuffles inside a group, so no lane may leave a pass early; a lane without work (unit >= units or j >= d) carries zeros
// through the pass and stores nothing.
#pragma once

#if defined(__HIPCC__)
#define HXG __host__ __device__ __forceinline__
#else
#define HXG inline
#endif

namespace hx {

constexpr unsigned GM_THREADS = 256;

// the next power of two >= d, 1 <= d <= 64
HXG unsigned gm_group(unsigned d)
{
  unsigned dp = 1;
  while (dp < d)
    dp *= 2;
  return dp;
}

// workgroups of a launch over `units` units, at most `cap`
HXG unsigned gm_blocks(unsigned long long units, unsigned dp, unsigned cap)
{
  const unsigned long long per = GM_THREADS / dp, b = (units + per - 1) / per;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// passes every thread of the launch runs
HXG unsigned gm_passes(unsigned long long units, unsigned dp, unsigned blocks)
{
  const unsigned long long per = (unsigned long long)blocks * (GM_THREADS / dp);
  return (unsigned)((units + per - 1) / per);
}

struct GmWork {
  unsigned long long unit;   // q nslots + s; the lane's words are unit d + j
  unsigned j;                // the lane inside its group
  bool owns;                 // unit < units and j < d: the lane loads v[j] and stores c[j]
};
HXG GmWork gm_work(unsigned block, unsigned tid, unsigned blocks, unsigned pass, unsigned long long units, unsigned d, unsigned dp)
{
  GmWork w;
  w.unit = ((unsigned long long)pass * blocks + block) * (GM_THREADS / dp) + tid / dp;
  w.j = tid & (dp - 1);
  w.owns = w.unit < units && w.j < d;
  return w;
}

}  // namespace hx
