// dgplace bulk release: client-releases-keys of many tasks at once (a cancelled graph) as
// parallel kernels on the stream engine's state between launches. Included by dgplace.hip
// after dgp_events.h; the host sequence is dgp_release_tasks' bulk path.
//
// k_ev_release_tasks (dgp_events.h) walks the plan on one lane; it stays the path for small
// plans and the yardstick for this one. The kernels here leave every array it writes with
// the same contents (DESIGN "Bulk release" has the argument). Each task is listed once, so
// its branch depends only on its state at entry: no kernel before k_rb_finish writes a task
// state, and every kernel reads the entry state. Separate launches stand in for grid-wide
// synchronisation:
//   k_rb_init / k_rb_scatter  pos[t] = the task's place in the plan (RB_NOPOS: not listed)
//   k_rb_classify             read-only: counts per entry state, the processing exits as
//                             (worker, place) keys, the fallback condition
//   k_rb_discard              cancel_discard's waiters, as atomic decrements
//   (queue)                   a stable select of qarr with RbKeep, then k_rb_queue_store
//   (exits)                   a radix sort of the exit keys, then k_rb_segments
//   k_rb_exits                one wave per worker: its exits in plan order (worker state only)
//   k_rb_flags                one wave per worker with an exit: check_idle_saturated as of its
//                             last exit's place in the plan
//   k_rb_globals              the global prefix dict, g_netocc, n_unrunnable
//   k_rb_clamp                waiters below zero (the serial "if waiters > 0") back to zero
//   k_rb_finish               per task: replicas, group counts, own counters, state
//   k_rb_refill               st::refill_queue, unchanged
// Every index is a task of the plan (checked < N by the host), a dependency of one (the
// graph's CSR), a worker read from proc_on (checked < W in k_rb_classify, which otherwise
// asks for the serial path) or a prefix (< P <= RB_PMAX, checked by the host).
#pragma once

namespace dgp {
namespace rb {

constexpr int32_t RB_NOPOS = INT32_MAX;
constexpr int RB_PMAX = 64;  // prefixes the per-block count tables hold
constexpr int RB_T = 256;    // threads of the per-task kernels

struct Info {
  int32_t n_exit;    // processing tasks of the plan
  int32_t n_queued;  // queued tasks of the plan
  int32_t n_nw;      // no-worker tasks of the plan
  int32_t fallback;  // a case outside what the bulk path proves: the serial kernel runs
  int32_t n_keep;    // queue entries the select kept
  int32_t pad;
};

struct Scratch {
  int32_t* pos;              // [N]
  int32_t* qtmp;             // [N] the compacted queue
  unsigned long long* key;   // [n] exit keys (worker << 32 | place), unsorted
  unsigned long long* skey;  // [n] ... sorted
  int64_t* ex_freed;         // [n] per sorted exit: network bytes it freed
  int32_t* ex_pfx;           // [n] ... its prefix, -1 for a long-running task (no count left)
  int32_t* seg_lo;           // [W] each worker's slice of the sorted exits
  int32_t* seg_hi;           // [W]
  Info* info;
};

// the select's predicate: a queue entry stays unless the plan lists it and it is queued
struct RbKeep {
  const int32_t* pos;
  const uint8_t* state;
  __device__ __forceinline__ bool operator()(const int32_t& t) const {
    return !(pos[t] != RB_NOPOS && state[t] == S_QUEUED);
  }
};

__device__ __forceinline__ bool rb_cancelled(uint8_t st) {
  return st == S_PROCESSING || st == S_WAITING || st == S_QUEUED || st == S_NO_WORKER;
}

__global__ void __launch_bounds__(RB_T) k_rb_init(const Dev* __restrict__ Dp, Scratch R) {
  const Dev& D = *Dp;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < D.N; t += stride) R.pos[t] = RB_NOPOS;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < D.W; w += stride) {
    R.seg_lo[w] = 0;
    R.seg_hi[w] = 0;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *R.info = Info{0, 0, 0, 0, 0, 0};
}

__global__ void __launch_bounds__(RB_T) k_rb_scatter(Scratch R, const int32_t* __restrict__ task, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) R.pos[task[i]] = i;
}

// Read-only pre-pass. The fallback: loss_exit_processing's scan-mode branch reads
// holds_any(d, x); serially that read sees d's replicas gone when the plan lists d's release
// (memory -> released) before the exit, and k_rb_exits runs before any replica is cleared.
__global__ void __launch_bounds__(RB_T) k_rb_classify(const Dev* __restrict__ Dp, Scratch R,
                                                      const int32_t* __restrict__ task, int n) {
  const Dev& D = *Dp;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = task[i];
  const uint8_t st = D.state[t];
  if (st == S_QUEUED) atomicAdd(&R.info->n_queued, 1);
  if (st == S_NO_WORKER) atomicAdd(&R.info->n_nw, 1);
  if (st != S_PROCESSING) return;
  const int x = D.proc_on[t];
  if (x < 0 || x >= D.W) {
    atomicOr(&R.info->fallback, 1);
    return;
  }
  const int k = atomicAdd(&R.info->n_exit, 1);
  R.key[k] = ((unsigned long long)(uint32_t)x << 32) | (uint32_t)i;
  if (ev::scan_mode(D, x)) {
    for (int64_t q = D.dep_ptr[t]; q < D.dep_ptr[t + 1]; q++) {
      const int d = D.dep_idx[q];
      if (R.pos[d] < i && D.state[d] == S_MEMORY) atomicOr(&R.info->fallback, 1);
    }
  }
}

// cancel_discard of every cancelled task. Serially task t at place i decrements waiters[d]
// of each dependency d that is not released at that moment and has waiters > 0. d is
// released at that moment iff it was at entry or the plan lists it before i (whatever its
// entry state, it is released from its own place on). The decrements commute; the floor at
// zero is k_rb_clamp's, and a cancelled d ends at 0 in k_rb_finish.
__global__ void __launch_bounds__(RB_T) k_rb_discard(const Dev* __restrict__ Dp, Scratch R,
                                                     const int32_t* __restrict__ task, int n) {
  const Dev& D = *Dp;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = task[i];
  if (!rb_cancelled(D.state[t])) return;
  for (int64_t q = D.dep_ptr[t]; q < D.dep_ptr[t + 1]; q++) {
    const int d = D.dep_idx[q];
    if (D.state[d] != S_RELEASED && R.pos[d] > i) atomicSub(&D.waiters[d], 1);
  }
}

__global__ void __launch_bounds__(RB_T) k_rb_clamp(const Dev* __restrict__ Dp) {
  const Dev& D = *Dp;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < D.N; t += stride)
    if (D.waiters[t] < 0) D.waiters[t] = 0;
}

// the compacted queue back into qarr[qhead, qhead + n_keep); a listed queued task that was
// not in the queue is ERR_BAD_STATE, as in the serial kernel
__global__ void __launch_bounds__(RB_T) k_rb_queue_store(const Dev* __restrict__ Dp, Scratch R, long long qhead,
                                                         long long qlen) {
  const Dev& D = *Dp;
  const long long keep = R.info->n_keep;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < keep && q < qlen; q += stride)
    D.qarr[qhead + q] = R.qtmp[q];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (qlen - keep != (long long)R.info->n_queued) set_error(D, ERR_BAD_STATE, -1);
    D.ctl->qlen = keep;
  }
}

// each worker's slice of the sorted exit keys
__global__ void __launch_bounds__(RB_T) k_rb_segments(Scratch R, int m) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= m) return;
  const int x = (int)(R.skey[k] >> 32);
  if (k == 0 || (int)(R.skey[k - 1] >> 32) != x) R.seg_lo[x] = k;
  if (k == m - 1 || (int)(R.skey[k + 1] >> 32) != x) R.seg_hi[x] = k + 1;
}

// WorkerState.remove_from_processing of every exit of worker x = blockIdx.x, in plan order:
// what loss_exit_processing(t, -1, false) writes of worker x's state. The global dict,
// g_netocc and check_idle_saturated are k_rb_globals' and k_rb_flags'. Lane 0 works (the
// needs_what functions of the event cascades are single-lane); no worker has two waves.
__global__ void __launch_bounds__(64) k_rb_exits(const Dev* __restrict__ Dp, Scratch R,
                                                 const int32_t* __restrict__ task) {
  const Dev& D = *Dp;
  const int x = blockIdx.x;
  if (threadIdx.x != 0) return;
  const int lo = R.seg_lo[x], hi = R.seg_hi[x];
  uint32_t* L = D.gw_needs_saved + (size_t)x * SNLW;
  for (int k = lo; k < hi; k++) {
    const int t = task[(uint32_t)R.skey[k]];
    const int p = D.prefix[t];
    int64_t freed = 0;
    for (int64_t q = D.dep_ptr[t]; q < D.dep_ptr[t + 1]; q++) {
      const int d = D.dep_idx[q];
      if (L[SNLW - 1] == SNL_OVF) {  // scan mode: needed iff not held and nobody else on x needs it
        if (!holds_any(D, d, x) && !needed_elsewhere(D, d, x, t)) freed += res_nb(D, d);
        continue;
      }
      bool present = false;  // "if dts in self.needs_what"
      for (int i = 0; i < SNLW - 1 && !present; i++) present = L[i] != 0 && (L[i] >> 8) == (uint32_t)d;
      if (!present && (int)(L[SNLW - 1] >> 8) > 0)
        for (int i = 0; i < SNXW && !present; i++) {
          const uint32_t e = D.gw_needs_ext[(size_t)x * SNXW + i];
          present = e != 0 && (e >> 8) == (uint32_t)d;
        }
      if (present) freed += sneeds_dec(D, x, d, t);
    }
    const int npw = D.w_nproc[x] - 1;
    if (npw == 0) sneeds_reset(D, x);
    const bool lr = (D.tdyn[t] & TD_LR) != 0;
    if (lr) {
      D.w_cap[x] -= 1;
      D.tdyn[t] &= (uint8_t)~TD_LR;
    } else {
      wdict_dec(D, x, p);
    }
    D.w_nproc[x] = npw;
    D.w_netocc[x] -= freed;
    D.proc_on[t] = -1;
    R.ex_freed[k] = freed;
    R.ex_pfx[k] = lr ? -1 : p;
  }
}

// check_idle_saturated of worker x = blockIdx.x after its last exit. Idle / saturated /
// idle_task_count membership is a flag per worker, so of the checks the serial kernel makes
// after each exit only the last one's result stays. It reads x's own occupancy and
// len(processing), final since k_rb_exits, and SchedulerState.total_occupancy at that place
// of the plan: the global prefix counts at entry less the exits listed up to there (a
// long-running one left the count earlier), g_netocc at entry less the bytes they freed.
// The sum runs in the global dict's insertion order; an entry that reached 0 adds
// duration * 0.0, which leaves the sum's bits as they are, so the dict is compacted later.
__global__ void __launch_bounds__(64) k_rb_flags(const Dev* __restrict__ Dp, Scratch R, int m) {
  const Dev& D = *Dp;
  const int x = blockIdx.x;
  const int lo = R.seg_lo[x], hi = R.seg_hi[x];
  if (lo >= hi) return;
  __shared__ long long s_cnt[RB_PMAX];
  __shared__ unsigned long long s_freed;
  const int lane = threadIdx.x;
  s_cnt[lane] = 0;  // RB_PMAX == 64 lanes
  if (lane == 0) s_freed = 0;
  __syncthreads();
  const uint32_t last = (uint32_t)R.skey[hi - 1];
  long long freed = 0;
  for (int k = lane; k < m; k += 64) {
    if ((uint32_t)R.skey[k] > last) continue;
    freed += R.ex_freed[k];
    const int p = R.ex_pfx[k];
    if (p >= 0) atomicAdd((unsigned long long*)&s_cnt[p], 1ull);
  }
  atomicAdd(&s_freed, (unsigned long long)freed);
  __syncthreads();
  if (lane != 0) return;
  Ctl* c = D.ctl;
  double tot = 0.0;
  for (int i = 0; i < c->g_plen; i++) {
    const int p = c->g_pfx[i];
    tot += prefix_duration(D, D.pdur_walk, p) * (double)(c->g_pcnt[i] - s_cnt[p]);
  }
  tot += (c->g_netocc - (double)(long long)s_freed) / (double)D.bandwidth;
  // walk_flags' rule with that total; the set sizes by atomics (one wave per worker)
  const double occ = occupancy(D, x, D.pdur_walk);
  const int64_t p = D.w_nproc[x];
  const int64_t nt = D.w_nthreads[x];
  const uint8_t fl = D.w_flags[x];
  const double avg = tot / (double)D.total_nthreads;
  bool idle = false, sat = false;
  if (fl & WF_PAUSED) {
  } else if (p < nt) {
    idle = true;
  } else {
    idle = occ < (double)nt * avg / 2;
  }
  if (!idle && p > nt && !(fl & WF_PAUSED)) {
    const double pending = occ * (double)(p - nt) / (double)(p * nt);
    if (0.4 < pending) sat = pending > 1.9 * avg;
  }
  if (idle != ((fl & WF_IDLE) != 0)) atomicAdd((unsigned long long*)&c->n_idle, idle ? 1ull : (unsigned long long)-1ll);
  if (sat != ((fl & WF_SAT) != 0)) atomicAdd((unsigned long long*)&c->n_sat, sat ? 1ull : (unsigned long long)-1ll);
  D.w_flags[x] = (uint8_t)((fl & ~(WF_IDLE | WF_SAT)) | (idle ? WF_IDLE : 0) | (sat ? WF_SAT : 0));
  itc_check(D, x, false);  // final state only; its counts are atomics already
}

// the global prefix dict less every exit that still counted, compacted once with its order
// kept (gdict_dec's delete-on-zero); g_netocc (integers below 2^53: exact in any order);
// the no-worker tasks out of unrunnable
__global__ void __launch_bounds__(RB_T) k_rb_globals(const Dev* __restrict__ Dp, Scratch R, int m) {
  const Dev& D = *Dp;
  __shared__ long long s_cnt[RB_PMAX];
  __shared__ unsigned long long s_freed;
  if (threadIdx.x < RB_PMAX) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_freed = 0;
  __syncthreads();
  long long freed = 0;
  for (int k = threadIdx.x; k < m; k += blockDim.x) {
    freed += R.ex_freed[k];
    const int p = R.ex_pfx[k];
    if (p >= 0) atomicAdd((unsigned long long*)&s_cnt[p], 1ull);
  }
  atomicAdd(&s_freed, (unsigned long long)freed);
  __syncthreads();
  if (threadIdx.x != 0) return;
  Ctl* c = D.ctl;
  int o = 0;
  for (int i = 0; i < c->g_plen; i++) {
    const int p = c->g_pfx[i];
    const long long v = c->g_pcnt[i] - s_cnt[p];
    if (v == 0 && s_cnt[p] != 0) continue;
    c->g_pfx[o] = p;
    c->g_pcnt[o] = v;
    o++;
  }
  c->g_plen = o;
  c->g_netocc -= (double)(long long)s_freed;
  c->n_unrunnable -= R.info->n_nw;
}

// per task, by its entry state: remove_all_replicas of a result, a cancelled task's own
// counters, the TaskGroup counts, the state
__global__ void __launch_bounds__(RB_T) k_rb_finish(const Dev* __restrict__ Dp, const int32_t* __restrict__ task,
                                                    int n) {
  const Dev& D = *Dp;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int t = task[i];
  const uint8_t st = D.state[t];
  const bool forgotten = (D.tflags[t] & TF_FORGOTTEN) != 0;
  if (st == S_RELEASED) {
    if (forgotten) atomicAdd((unsigned long long*)&D.g_relwait[D.group[t]], (unsigned long long)-1ll);
    return;
  }
  if (st == S_MEMORY) {
    const int64_t nb = st::nbv(D, D.res_nbytes[t]);
    for (int b = 0; b < D.WB; b++) {
      unsigned long long m = D.holders[(size_t)t * D.WB + b];
      D.holders[(size_t)t * D.WB + b] = 0;
      for (; m; m &= m - 1)
        atomicAdd((unsigned long long*)&D.w_nbytes[b * 64 + __builtin_ctzll(m)], (unsigned long long)(-nb));
    }
    D.tdyn[t] &= (uint8_t)~TD_MULTI;
    D.holder_of[t] = -1;
  } else if (rb_cancelled(st)) {
    if (st == S_PROCESSING) D.holder_of[t] = -1;
    if (st == S_WAITING) D.remaining[t] = ev::ERRED_REMAINING;
    D.waiters[t] = 0;  // ts.waiters = None
  } else {
    set_error(D, ERR_UNSUPPORTED, t);
    return;
  }
  const long long dg = (st != S_WAITING ? 1 : 0) - (forgotten ? 1 : 0);
  if (dg) atomicAdd((unsigned long long*)&D.g_relwait[D.group[t]], (unsigned long long)dg);
  D.state[t] = S_RELEASED;
}

__global__ void __launch_bounds__(64) k_rb_refill(const Dev* __restrict__ Dp, long long* placed) {
  const Dev& D = *Dp;
  __shared__ st::SCtl S;
  ev::ev_init(S);
  if (st::lane_id() == 0) *placed = 0;
  if (D.ctl->error) return;
  const long long m = st::refill_queue(D, S);
  if (st::lane_id() == 0) {
    *placed = m;
    if (S.error) set_error(D, S.error, S.err_task);
  }
}

}  // namespace rb
}  // namespace dgp
