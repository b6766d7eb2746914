// Rectangular linear sum assignment on the host (include/gapro_hip.h, gapro_lsap_solve): what the consumer's matcher
// hands to scipy.optimize (ISBNet isbnet/model/matcher.py:201-204), without the copy of the repeated matrix.
//
// Shortest augmenting paths (Jonker and Volgenant, "A shortest augmenting path algorithm for dense and sparse linear
// assignment problems", Computing 38, 1987) in the rectangular form of Crouse, "On implementing 2D rectangular
// assignment algorithms", IEEE Trans. AES 52(4), 2016: the side with fewer entries is the "workers", each of which is
// given a "job" of the other side.  Worker after worker, a Dijkstra search over the reduced costs
// c(w, j) - u[w] - v[j] finds the shortest alternating path from the new worker to an unassigned job, the duals u, v
// (float64) are moved so that the reduced costs stay non-negative and are zero on the assignment, and the assignment is
// flipped along the path.  O(n_workers^2 n_jobs).
//
// Ties: a search step closes, among the open jobs at the smallest distance, an unassigned one before an assigned one and
// the lowest index first.  Nothing here depends on the run: same input, same output.
// Host-only: no device, no HIP header.
#include <cmath>
#include <cstdint>
#include <limits>
#include <utility>
#include <vector>

#include "../../include/gapro_hip.h"

namespace {

// cost of (worker w, job j): the matrix with its columns repeated `dup` times, transposed when the rows are the jobs.
// The search scans one worker against every open job, so the given matrix (never the repeated one) is kept worker-major
// in float64, and the repeats are two small index tables.
struct CostView {
  std::vector<double> base;       // [distinct workers][distinct jobs]
  std::vector<int32_t> job_slot;  // [n_jobs] column of `base` of a job
  int32_t n_base_workers, n_base_jobs;
  CostView(const float* c, int64_t ld, int32_t n_rows, int32_t n_cols, int32_t dup, bool rows_are_jobs)
      : n_base_workers(rows_are_jobs ? n_cols : n_rows), n_base_jobs(rows_are_jobs ? n_rows : n_cols) {
    base.resize((size_t)n_base_workers * n_base_jobs);
    for (int32_t i = 0; i < n_rows; ++i)
      for (int32_t j = 0; j < n_cols; ++j)
        base[rows_are_jobs ? (size_t)j * n_rows + i : (size_t)i * n_cols + j] = (double)c[(int64_t)i * ld + j];
    const int32_t n_jobs = rows_are_jobs ? n_rows : dup * n_cols;
    job_slot.resize(n_jobs);
    for (int32_t j = 0; j < n_jobs; ++j) job_slot[j] = j % n_base_jobs;
  }
  const double* worker(int32_t w) const { return base.data() + (size_t)(w % n_base_workers) * n_base_jobs; }
};

// job_of[w] for every worker; n_workers <= n_jobs and every cost is finite, so every search ends in an unassigned job
void solve(const CostView& cost, int32_t n_workers, int32_t n_jobs, std::vector<int32_t>& job_of) {
  const int32_t* slot = cost.job_slot.data();
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> u(n_workers, 0.0), v(n_jobs, 0.0), dist(n_jobs);
  std::vector<int32_t> worker_of(n_jobs, -1), pred(n_jobs), open(n_jobs), reached;
  job_of.assign(n_workers, -1);
  reached.reserve(n_workers);
  for (int32_t cur = 0; cur < n_workers; ++cur) {
    for (int32_t j = 0; j < n_jobs; ++j) {
      dist[j] = inf;
      pred[j] = -1;
      open[j] = j;
    }
    reached.clear();  // the workers the search has scanned, `cur` among them
    int32_t n_open = n_jobs, w = cur, sink = -1;
    double min_val = 0.0;
    while (sink < 0) {
      reached.push_back(w);
      double lowest = inf;
      int32_t pick = -1;  // position in `open`
      const double* cw = cost.worker(w);
      const double uw = u[w];
      for (int32_t k = 0; k < n_open; ++k) {
        const int32_t j = open[k];
        const double r = min_val + cw[slot[j]] - uw - v[j];
        if (r < dist[j]) {
          dist[j] = r;
          pred[j] = w;
        }
        bool better = pick < 0 || dist[j] < lowest;
        if (!better && dist[j] == lowest) {  // a tie: an unassigned job first, then the lower index
          const int32_t best = open[pick];
          const bool free_j = worker_of[j] < 0, free_best = worker_of[best] < 0;
          better = free_j != free_best ? free_j : j < best;
        }
        if (better) {
          lowest = dist[j];
          pick = k;
        }
      }
      min_val = lowest;
      const int32_t j = open[pick];
      if (worker_of[j] < 0) sink = j;
      else w = worker_of[j];
      std::swap(open[pick], open[--n_open]);  // closed: its dist is final; the closed jobs are the tail of `open`
    }
    // the duals: every scanned worker and every closed job moves by what the search still had to go from it
    u[cur] += min_val;
    for (size_t k = 1; k < reached.size(); ++k) {
      const int32_t i = reached[k];
      u[i] += min_val - dist[job_of[i]];
    }
    for (int32_t k = n_open; k < n_jobs; ++k) {
      const int32_t j = open[k];
      v[j] -= min_val - dist[j];
    }
    // flip the assignment along the path back to `cur`
    for (int32_t j = sink;;) {
      const int32_t i = pred[j];
      worker_of[j] = i;
      std::swap(job_of[i], j);
      if (i == cur) break;
    }
  }
}

}  // namespace

extern "C" int gapro_lsap_solve(int32_t n_rows, int32_t n_cols, const float* cost, int64_t ld, int32_t dup,
                                int32_t* n_out, int32_t* rows, int32_t* cols) {
  if (n_rows < 1 || n_cols < 1 || dup < 1 || !cost || ld < n_cols || !n_out || !rows || !cols ||
      (int64_t)dup * n_cols > 0x7fffffffLL)
    return GAPRO_ERR_BAD_ARG;
  for (int32_t i = 0; i < n_rows; ++i)
    for (int32_t j = 0; j < n_cols; ++j)
      if (!std::isfinite(cost[(int64_t)i * ld + j])) return GAPRO_ERR_NOT_FINITE;
  const int32_t wide = dup * n_cols;
  const bool rows_are_jobs = n_rows > wide;
  const CostView view(cost, ld, n_rows, n_cols, dup, rows_are_jobs);
  std::vector<int32_t> job_of;
  if (!rows_are_jobs) {
    solve(view, n_rows, wide, job_of);
    for (int32_t i = 0; i < n_rows; ++i) {
      rows[i] = i;
      cols[i] = job_of[i] % n_cols;
    }
    *n_out = n_rows;
    return GAPRO_OK;
  }
  solve(view, wide, n_rows, job_of);  // worker = a repeated column, job = a row
  std::vector<int32_t> col_of(n_rows, -1);
  for (int32_t j = 0; j < wide; ++j) col_of[job_of[j]] = j % n_cols;
  int32_t n = 0;
  for (int32_t i = 0; i < n_rows; ++i)
    if (col_of[i] >= 0) {
      rows[n] = i;
      cols[n] = col_of[i];
      ++n;
    }
  *n_out = n;
  return GAPRO_OK;
}
