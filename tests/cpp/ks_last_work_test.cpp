// The work map of the fused last-digit transform + key switch (helib_amd/csrc/work_map.h: ks_last_work) compiled for
// the host: every (output row, batch element) goes to exactly one workgroup, and the workgroups of one row follow each
// other in an XCD's dispatch order (hardware places workgroup id on XCD id % 8).
// TEST INFRASTRUCTURE: built by tests/, never linked into the product library.
#include <cstddef>
#include <vector>

#include "../../helib_amd/csrc/work_map.h"

// 0: a bijection onto nrows x batch whose rows are contiguous runs per XCD; else a code saying what failed.
// *max_rows_per_xcd: the most rows any XCD touches (its key-row and twiddle footprint).
extern "C" int check_ks_last_work(unsigned nrows, unsigned batch, unsigned* max_rows_per_xcd)
{
  const unsigned nwg = nrows * batch;
  std::vector<unsigned char> seen(nwg, 0);
  for (unsigned id = 0; id < nwg; id++) {
    const hx::KsWork w = hx::ks_last_work(id, nrows, batch);
    if (w.row >= nrows || w.b >= batch)
      return 1;
    unsigned char& s = seen[(std::size_t)w.row * batch + w.b];
    if (s)
      return 2;
    s = 1;
  }
  for (unsigned char s : seen)
    if (!s)
      return 3;
  unsigned most = 0;
  for (unsigned x = 0; x < 8; x++) {
    // the XCD's workgroups in dispatch order: a row, once left, never comes back, and elements ascend inside it
    std::vector<unsigned char> left(nrows, 0);
    unsigned prev_row = ~0u, prev_b = 0, rows_here = 0;
    for (unsigned id = x; id < nwg; id += 8) {
      const hx::KsWork w = hx::ks_last_work(id, nrows, batch);
      if (w.row != prev_row) {
        if (left[w.row])
          return 4;
        if (prev_row != ~0u)
          left[prev_row] = 1;
        rows_here++;
      } else if (w.b != prev_b + 1) {
        return 5;
      }
      prev_row = w.row;
      prev_b = w.b;
    }
    most = rows_here > most ? rows_here : most;
  }
  if (max_rows_per_xcd)
    *max_rows_per_xcd = most;
  return 0;
}
