// dgplace state audit: read-only recount of the engine's resident state (dgp_audit_state,
// include/dgplace.h lists the rules and their reference lines). Included by dgplace.hip after
// dgp_events.h.
//
// Five grid-wide launches over the canonical HBM layout, none of which writes an engine field:
//   k_au_needs   one wave per worker: the needs_what table (line + overflow entries) checked
//                for shape, its network occupancy summed, its entries copied to scratch
//   k_au_queue   one thread per queue position: range, state, priority order, membership count
//   k_au_tasks   one thread per task: the per-task rules, and the recount of every aggregate
//                into HBM scratch by atomics (per worker, per (worker, prefix), per needs
//                entry, per group)
//   k_au_workers one thread per worker, per (worker, prefix) and per needs entry: the kept
//                aggregates against the recount; the workers' dicts summed per prefix
//   k_au_globals the global dict, the Ctl counters and the group counts against the sums
// A corrupt state is the input this code exists for: every index read from the state is
// range-checked before it is used (an out-of-range one is reported, never dereferenced), and
// the violation append is bounded by `cap` by construction (one atomic per wave reserves the
// positions; a record is stored only at a position below cap; the total still counts).
#pragma once

namespace dgp {
namespace audit {

using st::NLW;
using st::NXW;
using st::NL_OVF;

constexpr int NE = 64;  // needs entries per worker in scratch: NLW - 1 line + NXW overflow, padded to a wave
static_assert(NLW - 1 + NXW <= NE, "one lane per needs_what entry");

// scratch of one audit (device pointers into one arena the engine owns); zeroed before each
// run up to `out`
struct Scratch {
  int32_t* c_nproc;    // [W] tasks with proc_on == w
  int32_t* c_lr;       // [W] ... of which TD_LR
  int32_t* c_wp;       // [W][P] tasks processing on w with prefix p, not TD_LR
  int32_t* c_needs;    // [W][NE] recounted multiplicity of each needs entry
  uint32_t* n_ent;     // [W][NE] the worker's entries (task << 8 | count), 0: none / invalid
  int32_t* c_qseen;    // [N] times the task is in the queue
  int64_t* c_nbytes;   // [W] sum of get_nbytes over the rows with bit w
  int64_t* c_grp;      // [G] released or waiting, not forgotten
  int64_t* c_gsum;     // [P] sum of the workers' dict counts
  int64_t* c_tot;      // [0] idle [1] saturated [2] idle_task_count [3] its slots [4] scan-mode workers
  uint8_t* scan;       // [W] the worker's needs_what is in scan mode
  // inputs from the host
  const uint8_t* status;    // [W] 0 running, 1 paused, 2 removed (the engine's host copy)
  const int32_t* base_cap;  // [W] max(ceil(saturation * nthreads), 1), 0 under inf (rows::base_cap)
  // output
  unsigned long long* n_viol;
  dgp_violation* out;
  long long cap;
};

__device__ __forceinline__ int lane() { return (int)(threadIdx.x & 63); }

// append a violation for every lane with `bad`: one atomic per wave reserves the positions.
// Called from divergent code too (per-lane holder and dependency loops): __ballot counts the
// active lanes only and the leader is one of them, so the __shfl reads an active lane.
__device__ __forceinline__ void report(const Scratch& A, bool bad, int rule, int field, int64_t index, int64_t sub,
                                       int64_t dev, int64_t expct) {
  const unsigned long long m = __ballot(bad);
  if (!m) return;
  const int leader = __builtin_ctzll(m);
  unsigned long long base = 0;
  if (lane() == leader) base = atomicAdd(A.n_viol, (unsigned long long)__builtin_popcountll(m));
  base = __shfl(base, leader);
  if (!bad) return;
  const unsigned long long pos = base + (unsigned long long)__builtin_popcountll(m & ((1ull << lane()) - 1));
  if (pos >= (unsigned long long)A.cap) return;
  dgp_violation v;
  v.rule = rule;
  v.field = field;
  v.index = index;
  v.sub = sub;
  v.device_value = dev;
  v.expected_value = expct;
  A.out[pos] = v;
}

// one atomic per distinct key among the wave's lanes with `on` (keys repeat: a group, a worker)
__device__ __forceinline__ void aadd(int32_t* p, int32_t v) { atomicAdd(p, v); }
__device__ __forceinline__ void aadd(int64_t* p, int64_t v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }
template <class T>
__device__ __forceinline__ void wave_add(T* arr, bool on, int key, T val) {
  unsigned long long todo = __ballot(on);
  while (todo) {
    const int l = __builtin_ctzll(todo);
    const int k = __shfl(key, l);
    const bool mine = on && key == k;
    const unsigned long long peers = __ballot(mine);
    T sum = 0;
    for (unsigned long long p = peers; p; p &= p - 1) sum += __shfl(val, __builtin_ctzll(p));
    if (lane() == l) aadd(arr + k, sum);
    todo &= ~peers;
  }
}

__device__ __forceinline__ bool row_empty(const Dev& D, int t) {
  for (int b = 0; b < D.WB; b++)
    if (D.holders[(size_t)t * D.WB + b]) return false;
  return true;
}
__device__ __forceinline__ bool active_state(uint8_t s) {  // the states that keep a dependency's waiters entry
  return s == S_WAITING || s == S_QUEUED || s == S_PROCESSING || s == S_NO_WORKER;
}

// ---------------------------------------------------------------- needs_what tables
__global__ void __launch_bounds__(256) k_au_needs(const Dev* __restrict__ Dp, Scratch A) {
  const Dev& D = *Dp;
  const int ln = lane();
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwave = (int)((gridDim.x * blockDim.x) >> 6);
  for (int w = wave; w < D.W; w += nwave) {
    const uint32_t* L = D.gw_needs_saved + (size_t)w * NLW;
    const uint32_t ctl = L[NLW - 1];
    if (ctl == NL_OVF) {  // scan mode: not compared
      if (ln == 0) {
        A.scan[w] = 1;
        atomicAdd((unsigned long long*)&A.c_tot[4], 1ull);
      }
      continue;
    }
    uint32_t e = ln < NLW - 1 ? L[ln] : 0u;
    const int used = __builtin_popcountll(__ballot(ln < NLW - 1 && e != 0));
    const int count = (int)(ctl >> 8);
    // the overflow entries are read only while the count says some are in use (needs_inc / needs_dec)
    if (count > used && ln >= NLW - 1 && ln < NLW - 1 + NXW) e = D.gw_needs_ext[(size_t)w * NXW + (ln - (NLW - 1))];
    const int total = __builtin_popcountll(__ballot(e != 0));
    report(A, ln == 0 && total != count, DGP_AR_WORKER_NEEDS, DGP_AF_NEEDS_LEN, w, -1, count, total);
    const int d = (int)(e >> 8);
    bool ok = e != 0 && d < D.N && (e & 0xffu) != 0;
    bool dup = false;
    for (int j = 0; j < NE - 1; j++) {  // an earlier slot naming the same task
      const uint32_t ej = __shfl(e, j);
      dup = dup || (j < ln && ej != 0 && e != 0 && (ej >> 8) == (e >> 8));
    }
    report(A, e != 0 && (!ok || dup), DGP_AR_WORKER_NEEDS, DGP_AF_NEEDS_TASK, w, ln, (int64_t)e, -1);
    ok = ok && !dup;
    A.n_ent[(size_t)w * NE + ln] = ok ? e : 0u;
    int64_t nb = ok ? get_nbytes(D, d) : 0;  // _network_occ: get_nbytes of each entry once (:806-810)
    for (int o = 32; o; o >>= 1) nb += __shfl_xor(nb, o);
    const int64_t kept = D.w_netocc[w];
    report(A, ln == 0 && kept != nb, DGP_AR_WORKER_NEEDS, DGP_AF_NETOCC, w, -1, kept, nb);
  }
}

// ------------------------------------------------------------------------- queue
__global__ void __launch_bounds__(256) k_au_queue(const Dev* __restrict__ Dp, Scratch A) {
  const Dev& D = *Dp;
  const long long qh = D.ctl->qhead, ql = D.ctl->qlen;
  const bool bad_range = qh < 0 || ql < 0 || qh > D.N || ql > D.N || qh + ql > D.N;
  if (bad_range) {
    if (blockIdx.x == 0 && threadIdx.x < 64) {
      report(A, threadIdx.x == 0, DGP_AR_QUEUE, DGP_AF_QUEUE_RANGE, -1, 0, qh, 0);
      report(A, threadIdx.x == 0, DGP_AR_QUEUE, DGP_AF_QUEUE_RANGE, -1, 1, ql, 0);
    }
    return;
  }
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i0 = (long long)blockIdx.x * blockDim.x; i0 < ql; i0 += step) {
    const long long i = i0 + threadIdx.x;
    const bool in = i < ql;
    const int t = in ? D.qarr[qh + i] : -1;
    const bool valid = in && t >= 0 && t < D.N;
    bool bad = in && !valid;
    if (valid) {
      atomicAdd(&A.c_qseen[t], 1);
      bad = D.state[t] != S_QUEUED;
      if (!bad && i > 0) {  // HeapSet order: ascending priority
        const int tp = D.qarr[qh + i - 1];
        if (tp >= 0 && tp < D.N) bad = !(D.prio[tp] < D.prio[t]);
      }
    }
    report(A, bad, DGP_AR_QUEUE, DGP_AF_QUEUE_ENTRY, i, -1, t, -1);
  }
}

// ------------------------------------------------------------------------- tasks
__global__ void __launch_bounds__(256) k_au_tasks(const Dev* __restrict__ Dp, Scratch A) {
  const Dev& D = *Dp;
  const int W = D.W, WB = D.WB;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long t0 = (long long)blockIdx.x * blockDim.x; t0 < D.N; t0 += step) {
    const long long tl = t0 + threadIdx.x;
    const bool in = tl < D.N;
    const int t = in ? (int)tl : 0;
    const uint8_t s = in ? D.state[t] : (uint8_t)S_RELEASED;
    const uint8_t td = in ? D.tdyn[t] : (uint8_t)0;
    const uint8_t tf = in ? D.tflags[t] : (uint8_t)TF_FORGOTTEN;
    const int po = in ? D.proc_on[t] : -1;
    const bool proc = in && s == S_PROCESSING;
    const bool po_ok = po >= 0 && po < W;

    // TASK_PROC
    report(A, in && ((po >= 0) != proc || (proc && !po_ok)), DGP_AR_TASK_PROC, DGP_AF_PROC_ON, t, -1, po, -1);
    report(A, proc && po_ok && A.status[po] == 2, DGP_AR_TASK_PROC, DGP_AF_PROC_ON, t, po, po, -1);

    // the recount per worker and per (worker, prefix): every task that names the worker
    const bool on_w = in && po_ok;
    const int px = in ? D.prefix[t] : 0;
    wave_add(A.c_nproc, on_w, po, (int32_t)1);
    wave_add(A.c_lr, on_w && (td & TD_LR), po, (int32_t)1);
    if (on_w && proc && !(td & TD_LR) && px >= 0 && px < D.P) atomicAdd(&A.c_wp[(size_t)po * D.P + px], 1);

    // GROUP_COUNT
    const int g = in ? D.group[t] : 0;
    wave_add(A.c_grp, in && (s == S_RELEASED || s == S_WAITING) && !(tf & TF_FORGOTTEN) && g >= 0 && g < D.G, g,
             (int64_t)1);

    // QUEUE: exactly the queued tasks, each once
    const int seen = in ? A.c_qseen[t] : 0;
    const int want = s == S_QUEUED ? 1 : 0;
    report(A, in && seen != want, DGP_AR_QUEUE, DGP_AF_QUEUE_MEMBER, t, -1, seen, want);

    // TASK_HOLDERS, and the recount of w_nbytes
    int pop = 0, first = -1;
    if (in) {
      const int64_t nb = get_nbytes(D, t);
      for (int b = 0; b < WB; b++) {
        for (unsigned long long m = D.holders[(size_t)t * WB + b]; m; m &= m - 1) {
          const int w = b * 64 + __builtin_ctzll(m);
          pop++;
          if (first < 0) first = w;
          const bool okw = w < W;
          if (okw) atomicAdd((unsigned long long*)&A.c_nbytes[w], (unsigned long long)nb);
          report(A, !okw || A.status[w] == 2, DGP_AR_TASK_HOLDERS, DGP_AF_HOLDERS, t, w, 1, 0);
        }
      }
    }
    report(A, in && (pop != 0) != (s == S_MEMORY), DGP_AR_TASK_HOLDERS, DGP_AF_HOLDERS, t, -1, pop,
           s == S_MEMORY ? 1 : 0);
    // TD_MULTI selects the row over holder_of as who_has (holds_any): it must be set once the
    // row has more than one bit. Set with one bit or none (a replica removed again, a result
    // released by the stream kernel) it reads the same who_has, the row being exact in both forms
    report(A, in && pop > 1 && !(td & TD_MULTI), DGP_AR_TASK_HOLDERS, DGP_AF_MULTI, t, -1, 0, 1);
    if (in && s == S_MEMORY && pop != 0) {
      const int h = D.holder_of[t];
      const bool held = h >= 0 && h < W && ((D.holders[(size_t)t * WB + (h >> 6)] >> (h & 63)) & 1ull);
      report(A, !held, DGP_AR_TASK_HOLDERS, DGP_AF_HOLDER_OF, t, -1, h, first);
    }

    // TASK_REMAINING
    if (in && active_state(s)) {
      int missing = 0;
      for (int64_t k = D.dep_ptr[t]; k < D.dep_ptr[t + 1]; k++) missing += row_empty(D, D.dep_idx[k]) ? 1 : 0;
      const int rem = D.remaining[t];
      const bool bad = s == S_WAITING ? (rem != missing || rem <= 0) : (rem != 0 || missing != 0);
      report(A, bad, DGP_AR_TASK_REMAINING, DGP_AF_REMAINING, t, -1, rem, missing);
    }

    // TASK_WAITERS
    if (in && s == S_MEMORY) {
      int n = 0;
      for (int64_t k = D.dpt_ptr[t]; k < D.dpt_ptr[t + 1]; k++) {
        const int y = D.dpt_idx[k];
        n += active_state(D.state[y]) && !(D.tflags[y] & TF_FORGOTTEN) ? 1 : 0;
      }
      const int kept = D.waiters[t];
      report(A, kept != n, DGP_AR_TASK_WAITERS, DGP_AF_WAITERS, t, -1, kept, n);
    }

    // WORKER_NEEDS: the dependencies the worker does not hold, counted onto its entries.
    // Once a replica event was seen (EVF_MULTI) an entry may be missing or count low, as in the
    // reference: add_replica deletes the entry whatever its count (:831-834) and a later
    // remove_replica does not bring it back (:786-798), so a task placed while the worker held
    // the dependency is not counted; needs_dec / sneeds_dec accept exactly that under EVF_MULTI
    // (dgp_stream.h, dgp_device.h). The rule is then one-sided: no entry counts more tasks
    // than need it, and none exists for a dependency the worker holds.
    if (proc && po_ok && !A.scan[po]) {
      const uint32_t* E = A.n_ent + (size_t)po * NE;
      for (int64_t k = D.dep_ptr[t]; k < D.dep_ptr[t + 1]; k++) {
        const int d = D.dep_idx[k];
        if (holds(D, d, po)) continue;
        int slot = -1;
        for (int i = 0; i < NE - 1 && slot < 0; i++)
          if (E[i] != 0 && (int)(E[i] >> 8) == d) slot = i;
        if (slot >= 0) {
          atomicAdd(&A.c_needs[(size_t)po * NE + slot], 1);
          continue;
        }
        // no entry: reported once, by the first task on the worker that needs d, with the multiplicity
        int mult = 0, firstx = -1;
        for (int64_t q = D.dpt_ptr[d]; q < D.dpt_ptr[d + 1]; q++) {
          const int x = D.dpt_idx[q];
          if (D.state[x] == S_PROCESSING && D.proc_on[x] == po) {
            mult++;
            if (firstx < 0 || x < firstx) firstx = x;
          }
        }
        report(A, firstx == t && !(D.evf & EVF_MULTI), DGP_AR_WORKER_NEEDS, DGP_AF_NEEDS_COUNT, po, d, 0, mult);
      }
    }
  }
}

// ----------------------------------------------------------------------- workers
__device__ __forceinline__ int dict_len(int n) { return n < 0 ? 0 : (n > PMAX ? PMAX : n); }

__global__ void __launch_bounds__(256) k_au_workers(const Dev* __restrict__ Dp, Scratch A) {
  const Dev& D = *Dp;
  const int W = D.W, P = D.P;
  const long long step = (long long)gridDim.x * blockDim.x, tid0 = (long long)blockIdx.x * blockDim.x;
  // one thread per worker
  for (long long w0 = tid0; w0 < W; w0 += step) {
    const long long wl = w0 + threadIdx.x;
    const bool in = wl < W;
    const int w = in ? (int)wl : 0;
    const int np = in ? D.w_nproc[w] : 0, cnt = in ? A.c_nproc[w] : 0;
    report(A, in && np != cnt, DGP_AR_WORKER_NPROC, DGP_AF_NPROC, w, -1, np, cnt);
    const int cap = in ? D.w_cap[w] : 0, ecap = in ? A.base_cap[w] + A.c_lr[w] : 0;
    report(A, in && !D.sat_inf && cap != ecap, DGP_AR_WORKER_NPROC, DGP_AF_CAP, w, -1, cap, ecap);
    const int64_t nb = in ? D.w_nbytes[w] : 0, enb = in ? A.c_nbytes[w] : 0;
    report(A, in && nb != enb, DGP_AR_WORKER_NBYTES, DGP_AF_NBYTES, w, -1, nb, enb);
    // WORKER_FLAGS
    const uint8_t fl = in ? D.w_flags[w] : (uint8_t)0;
    const bool paused = in && A.status[w] != 0;
    uint8_t efl = (uint8_t)(fl & (WF_IDLE | WF_SAT));
    if (paused) efl = 0;
    if (!paused && np == 0) efl = WF_IDLE;
    if ((efl & WF_IDLE) && (efl & WF_SAT)) efl = (uint8_t)(efl & ~WF_SAT);
    const bool itc = in && !paused && (D.sat_inf || cap - np > 0);
    efl = (uint8_t)(efl | (itc ? WF_ITC : 0) | (paused ? WF_PAUSED : 0));
    report(A, in && fl != efl, DGP_AR_WORKER_FLAGS, DGP_AF_FLAGS, w, -1, fl, efl);
    const int64_t slots = in ? D.w_itcslots[w] : 0, eslots = itc && !D.sat_inf ? cap - np : 0;
    report(A, in && !D.sat_inf && slots != eslots, DGP_AR_WORKER_FLAGS, DGP_AF_ITCSLOTS, w, -1, slots, eslots);
    if (in) {
      if (fl & WF_IDLE) atomicAdd((unsigned long long*)&A.c_tot[0], 1ull);
      if (fl & WF_SAT) atomicAdd((unsigned long long*)&A.c_tot[1], 1ull);
      if (fl & WF_ITC) {
        atomicAdd((unsigned long long*)&A.c_tot[2], 1ull);
        atomicAdd((unsigned long long*)&A.c_tot[3], (unsigned long long)slots);
      }
    }
    // WORKER_DICT: the dict's shape; its counts go into the per-prefix sums
    const int plen = in ? D.w_plen[w] : 0;
    report(A, in && (plen < 0 || plen > PMAX), DGP_AR_WORKER_DICT, DGP_AF_DICT_LEN, w, -1, plen, dict_len(plen));
    const int n = dict_len(plen);
    for (int i = 0; i < PMAX; i++) {
      const bool slot = in && i < n;
      const int p = slot ? D.w_pfx[(size_t)w * PMAX + i] : 0;
      bool bad = slot && (p < 0 || p >= P);
      for (int j = 0; j < i && slot && !bad; j++) bad = D.w_pfx[(size_t)w * PMAX + j] == p;
      report(A, bad, DGP_AR_WORKER_DICT, DGP_AF_DICT_PREFIX, w, i, p, -1);
      if (slot && !bad) atomicAdd((unsigned long long*)&A.c_gsum[p], (unsigned long long)(long long)D.w_pcnt[(size_t)w * PMAX + i]);
    }
  }
  // one thread per (worker, prefix): the dict's count against the recount
  const long long WP = (long long)W * P;
  for (long long i0 = tid0; i0 < WP; i0 += step) {
    const long long i = i0 + threadIdx.x;
    const bool in = i < WP;
    const int w = in ? (int)(i / P) : 0, p = in ? (int)(i % P) : 0;
    const int n = in ? dict_len(D.w_plen[w]) : 0;
    int kept = 0;
    bool present = false;
    for (int q = 0; q < n && !present; q++)
      if (D.w_pfx[(size_t)w * PMAX + q] == p) {
        present = true;
        kept = D.w_pcnt[(size_t)w * PMAX + q];
      }
    const int ex = in ? A.c_wp[i] : 0;
    report(A, in && (present ? (kept <= 0 || kept != ex) : ex != 0), DGP_AR_WORKER_DICT, DGP_AF_DICT_COUNT, w, p,
           present ? kept : 0, ex);
  }
  // one thread per needs entry: its count against the recount
  const long long WE = (long long)W * NE;
  for (long long i0 = tid0; i0 < WE; i0 += step) {
    const long long i = i0 + threadIdx.x;
    const bool in = i < WE;
    const uint32_t e = in ? A.n_ent[i] : 0u;
    const int ex = in ? A.c_needs[i] : 0;
    // after a replica event an entry may count fewer tasks than need it, never more (see k_au_tasks)
    const int kept = (int)(e & 0xffu);
    report(A, e != 0 && ((D.evf & EVF_MULTI) ? kept > ex : kept != ex), DGP_AR_WORKER_NEEDS, DGP_AF_NEEDS_COUNT, i / NE, (int64_t)(e >> 8),
           (int64_t)(e & 0xffu), ex);
  }
}

// ----------------------------------------------------------------------- globals
__global__ void __launch_bounds__(256) k_au_globals(const Dev* __restrict__ Dp, Scratch A) {
  const Dev& D = *Dp;
  const Ctl* c = D.ctl;
  const long long step = (long long)gridDim.x * blockDim.x, tid0 = (long long)blockIdx.x * blockDim.x;
  for (long long g0 = tid0; g0 < D.G; g0 += step) {
    const long long g = g0 + threadIdx.x;
    const bool in = g < D.G;
    const int64_t kept = in ? D.g_relwait[g] : 0, ex = in ? A.c_grp[g] : 0;
    report(A, in && kept != ex, DGP_AR_GROUP_COUNT, DGP_AF_RELWAIT, g, -1, kept, ex);
  }
  if (blockIdx.x != 0) return;
  const int gl = c->g_plen;
  const int n = gl < 0 ? 0 : (gl > PMAX_G ? PMAX_G : gl);
  const int tid = (int)threadIdx.x;
  report(A, tid == 0 && gl != n, DGP_AR_GLOBAL_DICT, DGP_AF_DICT_LEN, -1, -1, gl, n);
  for (int i0 = 0; i0 < PMAX_G; i0 += (int)blockDim.x) {  // the dict's shape, one thread per slot
    const int i = i0 + tid;
    const bool slot = i < n;
    const int p = slot ? c->g_pfx[i] : 0;
    bool bad = slot && (p < 0 || p >= D.P);
    for (int j = 0; j < i && slot && !bad; j++) bad = c->g_pfx[j] == p;
    report(A, bad, DGP_AR_GLOBAL_DICT, DGP_AF_DICT_PREFIX, -1, i, p, -1);
  }
  for (int p0 = 0; p0 < D.P; p0 += (int)blockDim.x) {  // one thread per prefix: count against the workers' sum
    const int p = p0 + tid;
    const bool in = p < D.P;
    long long kept = 0;
    bool present = false;
    for (int q = 0; q < n && in && !present; q++)
      if (c->g_pfx[q] == p) {
        present = true;
        kept = c->g_pcnt[q];
      }
    const long long ex = in ? A.c_gsum[p] : 0;
    report(A, in && (present ? (kept <= 0 || kept != ex) : ex != 0), DGP_AR_GLOBAL_DICT, DGP_AF_DICT_COUNT, -1, p,
           present ? kept : 0, ex);
  }
  report(A, tid == 0 && c->n_idle != A.c_tot[0], DGP_AR_WORKER_FLAGS, DGP_AF_N_IDLE, -1, -1, c->n_idle, A.c_tot[0]);
  report(A, tid == 0 && c->n_sat != A.c_tot[1], DGP_AR_WORKER_FLAGS, DGP_AF_N_SAT, -1, -1, c->n_sat, A.c_tot[1]);
  report(A, tid == 0 && c->n_itc != A.c_tot[2], DGP_AR_WORKER_FLAGS, DGP_AF_N_ITC, -1, -1, c->n_itc, A.c_tot[2]);
  report(A, tid == 0 && !D.sat_inf && c->itc_slots != A.c_tot[3], DGP_AR_WORKER_FLAGS, DGP_AF_ITC_SLOTS, -1, -1,
         c->itc_slots, A.c_tot[3]);
}

// ============================================================ against the scheduler's rows
// dgp_audit_tasks / _workers / _globals: a dry run of the resync. The host normalises the rows
// exactly as dgp_sync_* does and stages what the resync would write; these kernels report
// every element the engine holds that differs from it (a field the resync would change).

// dev[idx ? idx[i] : i] & mask against expect[i] & mask, one thread per element. index =
// (idx ? idx[i / div] : i / div), sub = div > 1 ? i % div (a row of div elements) : sub1.
// `lim` (nullable, per row): only the first max(lim_dev[row], lim_exp[row]) elements of a row
// are compared (an insertion-ordered dict: the slots past its length are dead).
template <class T>
__global__ void __launch_bounds__(256) k_au_cmp(const T* __restrict__ dev, const T* __restrict__ expect,
                                                const int32_t* __restrict__ idx, long long n, int div, T mask, int rule,
                                                int field, int sub1, const int32_t* __restrict__ lim_dev,
                                                const int32_t* __restrict__ lim_exp, Scratch A) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i0 = (long long)blockIdx.x * blockDim.x; i0 < n; i0 += step) {
    const long long i = i0 + threadIdx.x;
    bool in = i < n;
    const long long row = in ? i / div : 0, col = in ? i % div : 0;
    const long long at = idx ? (long long)idx[row] : row;  // idx entries are range-checked by the host
    if (in && lim_dev) {
      const int a = lim_dev[at], b = lim_exp[row];
      in = col < (a > b ? a : b) && col < div;
    }
    const T d = in ? (T)(dev[at * div + col] & mask) : (T)0, x = in ? (T)(expect[i] & mask) : (T)0;
    report(A, in && d != x, rule, field, at, div > 1 ? col : sub1, (int64_t)d, (int64_t)x);
  }
}

// the queue as a sequence: Ctl.qlen and qarr[qhead + i] against the HeapSet order of the rows
__global__ void __launch_bounds__(256) k_au_row_queue(const Dev* __restrict__ Dp, const int32_t* __restrict__ expect,
                                                      long long n, Scratch A) {
  const Dev& D = *Dp;
  const long long qh = D.ctl->qhead, ql = D.ctl->qlen;
  const bool ok = qh >= 0 && ql >= 0 && qh + ql <= D.N;
  if (blockIdx.x == 0 && threadIdx.x < 64)
    report(A, threadIdx.x == 0 && ql != n, DGP_AR_ROW_GLOBALS, DGP_AF_QUEUE_LEN, -1, -1, ql, n);
  const long long m = ok && ql < n ? ql : (ok ? n : 0);
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i0 = (long long)blockIdx.x * blockDim.x; i0 < m; i0 += step) {
    const long long i = i0 + threadIdx.x;
    const bool in = i < m;
    const int d = in ? D.qarr[qh + i] : 0, x = in ? expect[i] : 0;
    report(A, in && d != x, DGP_AR_ROW_GLOBALS, DGP_AF_QUEUE_ENTRY, i, -1, d, x);
  }
}

// needs_what as a multiset: one wave per worker, a lane per device entry; the rows' entries
// (task << 8 | count, CSR) are matched one by one. A worker whose rows would send it to scan
// mode (more than NLW - 1 + NXW entries) compares nothing here.
__global__ void __launch_bounds__(256) k_au_row_needs(const Dev* __restrict__ Dp, const int64_t* __restrict__ ptr,
                                                      const uint32_t* __restrict__ ent, Scratch A) {
  const Dev& D = *Dp;
  const int ln = lane();
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwave = (int)((gridDim.x * blockDim.x) >> 6);
  for (int w = wave; w < D.W; w += nwave) {
    const long long k0 = ptr[w], m = ptr[w + 1] - k0;
    if (m > NLW - 1 + NXW) continue;
    const uint32_t* L = D.gw_needs_saved + (size_t)w * NLW;
    const uint32_t ctl = L[NLW - 1];
    if (ctl == NL_OVF) {  // the engine scans where the rows have a table
      report(A, ln == 0, DGP_AR_ROW_WORKERS, DGP_AF_NEEDS_LEN, w, -1, -1, m);
      continue;
    }
    uint32_t e = ln < NLW - 1 ? L[ln] : 0u;
    const int used = __builtin_popcountll(__ballot(ln < NLW - 1 && e != 0));
    if ((int)(ctl >> 8) > used && ln >= NLW - 1 && ln < NLW - 1 + NXW)
      e = D.gw_needs_ext[(size_t)w * NXW + (ln - (NLW - 1))];
    report(A, ln == 0 && (long long)(ctl >> 8) != m, DGP_AR_ROW_WORKERS, DGP_AF_NEEDS_LEN, w, -1, ctl >> 8, m);
    bool matched = false;
    for (long long k = 0; k < m; k++) {
      const uint32_t x = ent[k0 + k];
      const unsigned long long hit = __ballot(e != 0 && (e >> 8) == (x >> 8));
      const uint32_t d = hit ? __shfl(e, __builtin_ctzll(hit)) : 0u;
      if (hit && ln == __builtin_ctzll(hit)) matched = true;
      report(A, ln == 0 && d != x, DGP_AR_ROW_WORKERS, DGP_AF_NEEDS_COUNT, w, x >> 8, d & 0xffu, x & 0xffu);
    }
    report(A, e != 0 && !matched, DGP_AR_ROW_WORKERS, DGP_AF_NEEDS_COUNT, w, e >> 8, e & 0xffu, 0);
  }
}

// The task rows of dgp_audit_tasks (normalised and range-checked by the host, dgp_rows.h), one
// thread per row: every field k_sync_tasks would write against what the engine holds. What
// follows from a row comes from the function k_sync_tasks itself calls (rows::derive_task; its
// who_has words go to who[i * WB ..], scratch). The columns a kernel reads only in some states
// are compared for the rows in those states (include/dgplace.h).
__global__ void __launch_bounds__(256) k_au_row_tasks(const Dev* __restrict__ Dp, const rows::TaskRow* __restrict__ row,
                                                      long long n, const int32_t* __restrict__ holders,
                                                      unsigned long long* __restrict__ who, Scratch A) {
  const Dev& D = *Dp;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const rows::TaskRow r = row[i];
    const int t = r.t;
    const uint8_t s = r.state;
    unsigned long long* x = who + (size_t)i * D.WB;
    const rows::TaskDerived d = rows::derive_task(r, holders, D.default_data_size, D.WB, x);
    auto cmp = [&](bool on, int field, int64_t dev, int64_t expct, int64_t sub) {
      report(A, on && dev != expct, DGP_AR_ROW_TASKS, field, t, sub, dev, expct);
    };
    const uint8_t tf = D.tflags[t], td = D.tdyn[t];
    cmp(true, DGP_AF_STATE, D.state[t], s, -1);
    cmp(true, DGP_AF_WAITERS, D.waiters[t], r.waiters, -1);
    cmp(true, DGP_AF_PROC_ON, D.proc_on[t], r.proc_on, -1);
    cmp(true, DGP_AF_RES_NBYTES, D.res_nbytes[t], r.nbytes, -1);
    for (int b = 0; b < D.WB; b++)  // sub = the word
      cmp(true, DGP_AF_WHO_HAS, (int64_t)D.holders[(size_t)t * D.WB + b], (int64_t)x[b], b);
    cmp(true, DGP_AF_LR, td & TD_LR, d.tdyn & TD_LR, -1);
    cmp(true, DGP_AF_WANTED, tf & TF_WANTED, rows::task_flag_bits(r) & TF_WANTED, -1);
    cmp(true, DGP_AF_FORGOTTEN, tf & TF_FORGOTTEN, rows::task_flag_bits(r) & TF_FORGOTTEN, -1);
    cmp(s == S_WAITING || s == S_PROCESSING || s == S_QUEUED || s == S_NO_WORKER, DGP_AF_REMAINING, D.remaining[t],
        r.remaining, -1);
    cmp(s == S_MEMORY, DGP_AF_CUR_NBYTES, D.cur_nbytes[t], d.cur_nbytes, -1);
    cmp(s == S_PROCESSING || (s == S_MEMORY && r.hn == 1), DGP_AF_HOLDER_OF, D.holder_of[t], d.holder_of, -1);
    cmp(r.hn > 1, DGP_AF_MULTI, td & TD_MULTI, d.tdyn & TD_MULTI, -1);
  }
}

}  // namespace audit
}  // namespace dgp
