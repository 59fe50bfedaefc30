// Stand-alone driver of distributed_amd/csrc/dgp_rows.h (host only; test_rows_host.py builds and
// runs it): one good row set of each kind with the image it must give, and every malformed
// input of the resync with the refusal it must get. Exits 0 when all hold.
#include "../distributed_amd/csrc/dgp_rows.h"

#include <cstdio>
#include <cstring>
#include <type_traits>

using namespace dgp::rows;

static int failures = 0;

static void expect(const char* what, const char* got, const char* want) {
  if ((!got && !want) || (got && want && !strcmp(got, want))) return;
  printf("%s: got %s, want %s\n", what, got ? got : "(accepted)", want ? want : "(accepted)");
  failures++;
}
static void check(const char* what, bool ok) {
  if (!ok) printf("%s\n", what), failures++;
}

static const int32_t nthreads[4] = {1, 2, 4, 8};
static const uint8_t mirror[4] = {0, 0, 1, 2};  // worker 2 paused, worker 3 removed
static const Shape S{6, 4, 1, 3, 2, 1.1, false, 1024, nthreads, mirror};

struct Tasks {
  std::vector<int32_t> task{0, 2, 3, 5}, remaining{0, 0, 0, 2}, waiters{1, 0, 0, 0}, proc{-1, 1, -1, -1}, hidx{0, 3};
  std::vector<uint8_t> state{5, 2, 7, 1}, lr{0, 1, 0, 0}, wanted{1, 0, 0, 1};
  std::vector<int64_t> nbytes{-1, 10, -1, -1}, hptr{0, 2, 2, 2, 2};
  const char* run(TaskImage& img) const {
    return task_rows(S, (int64_t)task.size(), task.data(), state.data(), remaining.data(), waiters.data(), proc.data(),
                     nbytes.data(), lr.data(), wanted.data(), hptr.data(), hidx.data(), img);
  }
};

struct Workers {
  std::vector<int8_t> status{0, 0, 1, 2};
  std::vector<int32_t> nproc{1, 0, 0, 0}, nlr{1, 0, 0, 0}, plen{1, 0, 0, 0}, prefix, count, ntask{0, 5}, ncount{1, 255};
  std::vector<int64_t> netocc{7, 0, 0, 0}, nbytes{0, 9, 0, 0}, nptr{0, 2, 2, 2, 2};
  std::vector<uint8_t> idle{0, 1, 0, 0}, sat{0, 0, 0, 0};
  Workers() : prefix(4 * PD, 0), count(4 * PD, 0) { prefix[0] = 2, count[0] = 1; }
  const char* run(WorkerImage& img) const {
    return worker_rows(S, (int32_t)status.size(), status.data(), nproc.data(), nlr.data(), plen.data(), prefix.data(),
                       count.data(), netocc.data(), nbytes.data(), idle.data(), sat.data(), nptr.data(), ntask.data(),
                       ncount.data(), img);
  }
};

struct Globals {
  std::vector<int32_t> gp{1, 0}, queued{4, 1}, lastw{-1, 3};
  std::vector<int64_t> gc{2, 1}, relw{1, 1}, left{0, 0};
  std::vector<double> dur{1, 2, 3}, mx{1, 2, 3};
  double bandwidth = 1e8;
  const char* run() const {
    return global_rows(S, (int32_t)gp.size(), gp.data(), gc.data(), (int64_t)queued.size(), queued.data(), dur.data(),
                       mx.data(), bandwidth, relw.data(), left.data(), lastw.data());
  }
};

template <class Rows, class F>
static const char* altered(F&& change) {
  Rows r;
  change(r);
  if constexpr (std::is_same<Rows, Tasks>::value) {
    TaskImage img;
    return r.run(img);
  } else if constexpr (std::is_same<Rows, Workers>::value) {
    WorkerImage img;
    return r.run(img);
  } else {
    return r.run();
  }
}

int main() {
  {  // the good rows and their images
    TaskImage img;
    expect("good tasks", Tasks().run(img), nullptr);
    const Tasks t;
    check("task image: rows", img.rows.size() == 4 && img.lr_any);
    check("task image: forgotten folds to released", img.rows[2].state == S_RELEASED && img.rows[2].forgotten == 1 &&
                                                         task_flag_bits(img.rows[2]) == TF_FORGOTTEN);
    check("task image: proc_on only when processing", img.rows[1].proc_on == 1 && img.rows[0].proc_on == -1);
    check("task image: wanted", task_flag_bits(img.rows[0]) == TF_WANTED && task_flag_bits(img.rows[1]) == 0);
    uint64_t who[1];
    TaskDerived d = derive_task(img.rows[0], t.hidx.data(), S.default_data_size, S.WB, who);
    check("derived: two holders", who[0] == 9 && d.holder_of == 0 && d.tdyn == TD_MULTI && d.cur_nbytes == 1024);
    d = derive_task(img.rows[1], t.hidx.data(), S.default_data_size, S.WB, who);
    check("derived: processing", who[0] == 0 && d.holder_of == 1 && d.tdyn == TD_LR && d.cur_nbytes == -1);
    WorkerImage w;
    expect("good workers", Workers().run(w), nullptr);
    check("worker image: cap", w.cap == std::vector<int32_t>({3, 3, 5, 9}));
    check("worker image: flags", w.flags == std::vector<uint8_t>({WF_ITC, WF_IDLE | WF_ITC, WF_PAUSED, WF_PAUSED}));
    check("worker image: slots and totals", w.slots == std::vector<int64_t>({2, 3, 0, 0}) && w.tot[0] == 1 &&
                                                w.tot[1] == 0 && w.tot[2] == 2 && w.tot[3] == 5);
    check("worker image: dict", w.plen[0] == 1 && w.pfx[0] == 2 && w.pcnt[0] == 1 && w.pfx.size() == 4u * PMAX);
    check("worker image: status", w.status == std::vector<uint8_t>({0, 0, 1, 2}) && w.paused_any && w.lr_any);
    check("worker image: needs", w.needs_ptr == std::vector<int64_t>({0, 2, 2, 2, 2}) &&
                                     w.needs == std::vector<uint32_t>({1u, (5u << 8) | 255u}));
    expect("good globals", Globals().run(), nullptr);
    check("cap rule", base_cap(1.1, false, 1) == 2 && base_cap(0.1, false, 1) == 1 && base_cap(1.1, true, 8) == 0);
  }
  // what the resync refuses
  expect("task id", altered<Tasks>([](Tasks& r) { r.task[0] = 6; }), "task / state / holder_ptr");
  expect("state 8", altered<Tasks>([](Tasks& r) { r.state[0] = 8; }), "task / state / holder_ptr");
  expect("holder_ptr", altered<Tasks>([](Tasks& r) { r.hptr[1] = -1; }), "task / state / holder_ptr");
  expect("holder", altered<Tasks>([](Tasks& r) { r.hidx[1] = 4; }), "holder out of range");
  expect("processing", altered<Tasks>([](Tasks& r) { r.proc[1] = -1; }), "processing task without a worker");
  expect("status 3", altered<Workers>([](Workers& r) { r.status[0] = 3; }), "status");
  expect("plen 9", altered<Workers>([](Workers& r) { r.plen[0] = 9; }), "more than 8 prefixes on a worker");
  expect("prefix = P", altered<Workers>([](Workers& r) { r.prefix[0] = 3; }), "prefix id");
  expect("idle paused", altered<Workers>([](Workers& r) { r.idle[2] = 1; }),
         "a worker that is not running is neither idle nor saturated");
  expect("removed returns", altered<Workers>([](Workers& r) { r.status[3] = 1; }), "a removed worker returns");
  expect("needs count 0", altered<Workers>([](Workers& r) { r.ncount[0] = 0; }), "needs_what entry");
  expect("needs count 256", altered<Workers>([](Workers& r) { r.ncount[1] = 256; }), "needs_what entry");
  expect("needs task = N", altered<Workers>([](Workers& r) { r.ntask[0] = 6; }), "needs_what entry");
  expect("needs_ptr", altered<Workers>([](Workers& r) { r.nptr[1] = -1; }), "needs_ptr");
  expect("g_plen", altered<Globals>([](Globals& r) { r.gp.assign(PMAX_G + 1, 0), r.gc.assign(PMAX_G + 1, 1); }),
         "bad arguments");
  expect("g prefix = P", altered<Globals>([](Globals& r) { r.gp[0] = 3; }), "prefix id");
  expect("queued = N", altered<Globals>([](Globals& r) { r.queued[0] = 6; }), "queued task");
  expect("last worker = W", altered<Globals>([](Globals& r) { r.lastw[0] = 4; }), "last worker");
  expect("bandwidth 0", altered<Globals>([](Globals& r) { r.bandwidth = 0; }), "bad arguments");
  if (failures) return 1;
  printf("rows ok\n");
  return 0;
}
