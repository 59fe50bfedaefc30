// dgplace -- the resync rows, normalised once (host only: plain C++17, nothing from HIP).
//
// dgp_sync_tasks / _workers / _globals write the scheduler's state into the engine and
// dgp_audit_tasks / _workers / _globals compare the engine against the same rows. Both take
// their rows through the functions below: each checks the ABI arguments of its row kind and
// either refuses -- it returns the message stem, which the caller prefixes with its own name --
// or fills the image of what the resync writes. The resync applies the image, the audit
// compares against it, so the two cannot disagree. Nothing here reads or changes the engine:
// the few quantities the rules depend on come in through `Shape`.
#ifndef DGP_ROWS_H  // (a guard, not #pragma once: the header is also compiled on its own)
#define DGP_ROWS_H

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define DGP_ROWS_HD __host__ __device__
#else
#define DGP_ROWS_HD
#endif

namespace dgp {
namespace rows {

// The layout and flag values of dgp_device.h / dgp_stream.h that the rules name (dgplace.hip
// asserts that they are equal).
constexpr int PD = 8;        // prefixes in a worker row of the ABI
constexpr int PMAX = 8;      // ... and the stride of the engine's per-worker dict
constexpr int PMAX_G = 64;   // prefixes in the global dict
constexpr int NLW = 12;      // needs_what: NLW - 1 entries in the line, then NXW overflow entries,
constexpr int NXW = 52;      // then scan mode
constexpr uint8_t S_RELEASED = 0, S_PROCESSING = 2, S_MEMORY = 5, S_FORGOTTEN = 7;  // 7: the ABI's row state only
constexpr uint8_t TF_WANTED = 1, TF_FORGOTTEN = 4;
constexpr uint8_t WF_IDLE = 1, WF_SAT = 2, WF_ITC = 4, WF_PAUSED = 8;
constexpr uint8_t TD_LR = 1, TD_MULTI = 2;

// what the rules read of the engine
struct Shape {
  int64_t N;  // tasks
  int W, WB, P, G;
  double saturation;
  bool sat_inf;
  int64_t default_data_size;
  const int32_t* nthreads;  // [W]
  const uint8_t* status;    // [W] the host's status column: 0 running, 1 paused, 2 removed
};

// _task_slots_available (:8765) without the long-running tasks: the one cap rule
// (dgp_set_workers refuses nthreads <= 0)
inline int32_t base_cap(double saturation, bool sat_inf, int32_t nthreads) {
  return sat_inf ? 0 : std::max((int32_t)std::ceil(saturation * nthreads), (int32_t)1);
}

// ----------------------------------------------------------------------------------- tasks
// One task row as the resync writes it; the device reads this layout (ev::SyncTask).
struct TaskRow {
  int32_t t, proc_on, remaining, waiters;
  int64_t nbytes;  // TaskState.nbytes (raw: -1 = never reported)
  int32_t hp, hn;  // who_has: holders [hp, hp + hn) of the holder list
  uint8_t state, lr, forgotten, wanted;
  int32_t pad;
};
static_assert(sizeof(TaskRow) == 40, "TaskRow layout is shared with the device");

struct TaskImage {
  std::vector<TaskRow> rows;
  bool lr_any = false;
};

// what follows from a row: written by k_sync_tasks, compared by dgp_audit_tasks
struct TaskDerived {
  int64_t cur_nbytes;
  int32_t holder_of;
  uint8_t tdyn;
};
// ... and the row's who_has words into who_has[0, WB)
template <class Word>
DGP_ROWS_HD inline TaskDerived derive_task(const TaskRow& r, const int32_t* holders, int64_t default_data_size, int WB,
                                           Word* who_has) {
  for (int b = 0; b < WB; b++) who_has[b] = 0;
  int first = -1;
  for (int k = 0; k < r.hn; k++) {
    const int w = holders[r.hp + k];
    who_has[w >> 6] |= (Word)1 << (w & 63);
    if (first < 0) first = w;
  }
  TaskDerived d;
  d.cur_nbytes = r.state == S_MEMORY ? (r.nbytes >= 0 ? r.nbytes : default_data_size) : -1;
  d.holder_of = r.state == S_PROCESSING ? r.proc_on : first;
  d.tdyn = (uint8_t)((r.lr ? TD_LR : 0) | (r.hn > 1 ? TD_MULTI : 0));
  return d;
}

inline const char* task_rows(const Shape& s, int64_t n, const int32_t* task, const uint8_t* state,
                             const int32_t* remaining, const int32_t* waiters, const int32_t* processing_on,
                             const int64_t* nbytes, const uint8_t* long_running, const uint8_t* wanted,
                             const int64_t* holder_ptr, const int32_t* holder_idx, TaskImage& out) {
  if (n < 0 || (n > 0 && (!task || !state || !remaining || !waiters || !processing_on || !nbytes || !long_running ||
                          !wanted || !holder_ptr)))
    return "bad rows";
  out = TaskImage{};
  if (n == 0) return nullptr;
  const int64_t H = holder_ptr[n];
  if (holder_ptr[0] != 0 || H < 0 || (H > 0 && !holder_idx)) return "holder_ptr";
  out.rows.resize((size_t)n);
  for (int64_t i = 0; i < n; i++) {
    const int32_t t = task[i];
    if (t < 0 || t >= s.N || state[i] > S_FORGOTTEN || holder_ptr[i + 1] < holder_ptr[i])
      return "task / state / holder_ptr";
    if (state[i] == S_PROCESSING && (processing_on[i] < 0 || processing_on[i] >= s.W))
      return "processing task without a worker";
    for (int64_t k = holder_ptr[i]; k < holder_ptr[i + 1]; k++)
      if (holder_idx[k] < 0 || holder_idx[k] >= s.W) return "holder out of range";
    TaskRow& r = out.rows[(size_t)i];
    r = TaskRow{};
    r.t = t;
    r.proc_on = state[i] == S_PROCESSING ? processing_on[i] : -1;
    r.remaining = remaining[i];
    r.waiters = waiters[i];
    r.nbytes = nbytes[i];
    r.hp = (int32_t)holder_ptr[i];
    r.hn = (int32_t)(holder_ptr[i + 1] - holder_ptr[i]);
    // state 7 = forgotten (:2853): the row stays, released, flagged so that nothing walks it as
    // a dependent any more (_propagate_forgotten drops it from its dependencies' dependents)
    r.forgotten = state[i] == S_FORGOTTEN ? 1 : 0;
    r.state = r.forgotten ? S_RELEASED : state[i];
    r.lr = long_running[i] ? 1 : 0;
    r.wanted = wanted[i] ? 1 : 0;  // who_wants (TF_WANTED) rides on the task flags
    out.lr_any = out.lr_any || r.lr;
  }
  return nullptr;
}

// the two task-flag bits a row decides
DGP_ROWS_HD inline uint8_t task_flag_bits(const TaskRow& r) {
  return (uint8_t)((r.wanted ? TF_WANTED : 0) | (r.forgotten ? TF_FORGOTTEN : 0));
}

// --------------------------------------------------------------------------------- workers
struct WorkerImage {
  std::vector<int32_t> cap, plen, pfx, pcnt;  // pfx / pcnt: rows of PMAX
  std::vector<uint8_t> flags, status;         // status: the host's new status column
  std::vector<int64_t> slots;                 // idle_task_count slots
  int64_t tot[4] = {0, 0, 0, 0};              // Ctl: n_idle, n_sat, n_itc, itc_slots
  bool paused_any = false, lr_any = false;
  // needs_what, (task << 8) | count, as a CSR over the workers. A row past the line and the
  // overflow (scan mode) keeps its length and holds zeros: its entries are neither checked
  // nor written nor compared.
  std::vector<int64_t> needs_ptr;
  std::vector<uint32_t> needs;
};

inline bool scan_mode(int64_t n_needs) { return n_needs > (NLW - 1) + NXW; }

inline const char* worker_rows(const Shape& s, int32_t n_workers, const int8_t* status, const int32_t* nproc,
                               const int32_t* n_long_running, const int32_t* plen, const int32_t* prefix,
                               const int32_t* count, const int64_t* netocc, const int64_t* nbytes, const uint8_t* idle,
                               const uint8_t* saturated, const int64_t* needs_ptr, const int32_t* needs_task,
                               const int32_t* needs_count, WorkerImage& out) {
  const int W = s.W;
  if (n_workers != W || !status || !nproc || !n_long_running || !plen || !prefix || !count || !netocc || !nbytes ||
      !idle || !saturated || !needs_ptr)
    return "one row per engine worker";
  out = WorkerImage{};
  out.cap.resize(W);
  out.plen.resize(W);
  out.pfx.assign((size_t)W * PMAX, 0);
  out.pcnt.assign((size_t)W * PMAX, 0);
  out.flags.resize(W);
  out.status.resize(W);
  out.slots.assign(W, 0);
  out.needs_ptr.assign((size_t)W + 1, 0);
  for (int w = 0; w < W; w++) {
    if (status[w] < 0 || status[w] > 2) return "status";
    if (plen[w] < 0 || plen[w] > PD) return "more than 8 prefixes on a worker";
    const bool running = status[w] == 0;
    if (!running && (idle[w] || saturated[w])) return "a worker that is not running is neither idle nor saturated";
    if (status[w] != 2 && s.status[w] == 2) return "a removed worker returns";
    out.status[w] = (uint8_t)status[w];
    out.paused_any = out.paused_any || !running;
    out.lr_any = out.lr_any || n_long_running[w] > 0;
    out.cap[w] = base_cap(s.saturation, s.sat_inf, s.nthreads[w]) + (s.sat_inf ? 0 : n_long_running[w]);
    out.plen[w] = plen[w];
    for (int i = 0; i < plen[w]; i++) {
      if (prefix[(size_t)w * PD + i] < 0 || prefix[(size_t)w * PD + i] >= s.P) return "prefix id";
      out.pfx[(size_t)w * PMAX + i] = prefix[(size_t)w * PD + i];
      out.pcnt[(size_t)w * PMAX + i] = count[(size_t)w * PD + i];
    }
    const bool itc = running && (s.sat_inf || out.cap[w] - nproc[w] > 0);
    out.flags[w] = (uint8_t)((idle[w] ? WF_IDLE : 0) | (saturated[w] ? WF_SAT : 0) | (itc ? WF_ITC : 0) |
                             (running ? 0 : WF_PAUSED));
    out.slots[w] = itc && !s.sat_inf ? out.cap[w] - nproc[w] : 0;
    out.tot[0] += idle[w] ? 1 : 0;
    out.tot[1] += saturated[w] ? 1 : 0;
    out.tot[2] += itc ? 1 : 0;
    out.tot[3] += out.slots[w];
    const int64_t k0 = needs_ptr[w], k1 = needs_ptr[w + 1], m = k1 - k0;
    if (k1 < k0 || (m > 0 && (!needs_task || !needs_count))) return "needs_ptr";
    out.needs_ptr[w + 1] = out.needs_ptr[w] + m;
    if (scan_mode(m)) {
      out.needs.resize(out.needs.size() + (size_t)m, 0u);
      continue;
    }
    for (int64_t k = 0; k < m; k++) {
      const int32_t d = needs_task[k0 + k], c = needs_count[k0 + k];
      if (d < 0 || d >= s.N || c <= 0 || c > 255) return "needs_what entry";
      out.needs.push_back(((uint32_t)d << 8) | (uint32_t)c);
    }
  }
  return nullptr;
}

// --------------------------------------------------------------------------------- globals
// the argument check only: what the resync writes is the arguments themselves
inline const char* global_rows(const Shape& s, int32_t g_plen, const int32_t* g_prefix, const int64_t* g_count,
                               int64_t n_queued, const int32_t* queued, const double* duration_average,
                               const double* max_exec_time, double bandwidth, const int64_t* group_released_waiting,
                               const int64_t* group_left, const int32_t* group_last_worker) {
  if (g_plen < 0 || g_plen > PMAX_G || (g_plen > 0 && (!g_prefix || !g_count)) || n_queued < 0 || n_queued > s.N ||
      (n_queued > 0 && !queued) || !duration_average || !max_exec_time || !(bandwidth > 0) ||
      !group_released_waiting || !group_left || !group_last_worker)
    return "bad arguments";
  for (int i = 0; i < g_plen; i++)
    if (g_prefix[i] < 0 || g_prefix[i] >= s.P) return "prefix id";
  for (int64_t i = 0; i < n_queued; i++)
    if (queued[i] < 0 || queued[i] >= s.N) return "queued task";
  for (int g = 0; g < s.G; g++)
    if (group_last_worker[g] < -1 || group_last_worker[g] >= s.W) return "last worker";
  return nullptr;
}

}  // namespace rows
}  // namespace dgp

#endif  // DGP_ROWS_H
