// ns_route.cpp — the reference's per-token device graph: deferred, fused, verified, replayed (round 5: replay; round 6: one route per device
// queue, the deferred-launch window for evaluations that are not replayed, the fp16 kv mirror inside the plan, re-evaluation of a token)
//
// What it serves: a reference tree built with its device switch (-DNS_SYCL) rebuilds its graph every token
// (/root/reference/neural_speed/models/llama/llama.cpp:148) and its executor issues the ~780 nodes one by one
// (core/ne_layers.c:11915-12028: bestla_parallel_for per node, strictly serial, :11973).  On this library's bestla_device_* set every
// node is one HIP launch, ~3.5 us of host time each: an unchanged Model.generate() was bound by the HOST (242-297 tok/s),
// not by the GPU.  The reference's executor cannot be changed; what it calls can:
//   * every launch of the route (bestla_device_f32f32_forward and the pointer-level functions behind glue/ne_bestla_hip_device.c) is
//     described by one plain RouteOp and handed to route_submit();
//   * NOTHING is launched when it is handed over.  The reference's executor only synchronises where data crosses to the host
//     (bestla_device_sync / _memcpy: the embeddings go in and the logits come out there, ne_layers.c:8345-8346), so an evaluation's launches
//     are collected until then (the WINDOW) and go out as the library's fused forms — the reference builds its graph from single operators
//     (llama.cpp:203-330), a window knows what follows each of them (optimize() below).  Round 5 had these fusions under replay only: a 1500-token
//     prompt was ~800 single launches (58 ms), the first tokens of every generation too;
//   * two consecutive tokens whose op sequences agree in everything except ONE moving value per op (RoPE's n_past, the kv-cache cell a
//     cpy writes, the attention's context length) make a PLAN: the sequence is cut into segments of a few dozen ops, each captured into
//     a HIP graph in which a moving value is base + delta * (*k) — k one device word that the first segment increments (Affine, ns_common.h);
//   * from then on a token's ops are only COMPARED with the plan (a memcmp per node: ~0.1 us instead of a launch); when the last op of a
//     segment has matched, that segment's graph is launched (the GPU starts on a token while the executor is still walking it) — nothing of a
//     plan is launched before it is verified, so a token that deviates (another prompt, a context shift, a different batch) falls back
//     without side effects: what it handed over so far goes through the window, the plan is dropped, and the next agreeing tokens make a new one
//     (after consecutive fall-backs with a growing pause: interleaved sequences must not pay a capture every other token).
// One Route per device queue (bestla_create_device): two models — or a draft and a target model — in one process keep separate traces and plans.
// NS_DEVICE_REPLAY=0 turns plans off, NS_ROUTE_WINDOW=0 the window (every op launches as it comes: the round-4 behaviour).
// The route's code by role (shared declarations: ns_route_int.h; the fields of a RouteOp: ns_route_op.h):
//   ns_route_fuse.cpp  what a token's launches are — the diff of two tokens, the fusions, the segment cut: pure host code
//   ns_route_exec.cpp  issuing one launch
//   this file          the per-queue state machine: submit / verify / replay, bail-out, window flush, sync points, the input stash, capture
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <unordered_set>
#include <vector>

#include "../../include/ns_bestla.h"
#include "ns_common.h"
#include "ns_device_plan.h"
#include "ns_route_int.h"

namespace ns {
namespace {

__global__ void route_count_kernel(int* k) { *k += 1; }

struct Segment : SegmentCut {
  hipGraphExec_t exec = nullptr;
};
// a copy that brought an evaluation's input tensor (the embeddings): kept on the device so that the evaluation can be issued again
struct Stash {
  void* dst;
  size_t bytes, off;
};
long long now_us() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (long long)ts.tv_sec * 1000000ll + ts.tv_nsec / 1000;
}
// NS_ROUTE_TIMING=1 (diagnostics): events around a replayed token's segments -> GPU span per token; host marks of a token's phases; printed when the
// route detaches.  Every mark, sum and line of it is here.
enum { TM_PREV_END = 0, TM_FIRST_OP, TM_FIRST_LAUNCH, TM_LAST_LAUNCH, TM_SYNC_IN, TM_SYNC_OUT, TM_N };
struct RouteTiming {
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool ev_pending = false;
  double gpu_ms_sum = 0.0, host_us_sum = 0.0;
  long long gpu_tokens = 0;
  long long tm[TM_N] = {0, 0, 0, 0, 0, 0};
  double tm_sum[TM_N] = {0, 0, 0, 0, 0, 0};  // [i]: us from mark i to mark i + 1 (the last: sync out -> end of the token's last copy), replayed tokens
  long long tm_tokens = 0;
  bool replayed = false;
  bool prev_pending = false;
  long long win_t0 = 0, win_ops = 0, win_launches = 0, win_issue_us = 0;  // the last window that went out

  void first_op() { tm[TM_FIRST_OP] = now_us(), replayed = false; }
  void first_segment(hipStream_t st) {
    if (!ev0) (void)hipEventCreate(&ev0), (void)hipEventCreate(&ev1);
    (void)hipEventRecord(ev0, st);
    tm[TM_FIRST_LAUNCH] = now_us();
  }
  void last_segment(hipStream_t st) {
    (void)hipEventRecord(ev1, st);
    ev_pending = true;
    tm[TM_LAST_LAUNCH] = now_us();
    host_us_sum += double(tm[TM_LAST_LAUNCH] - tm[TM_FIRST_LAUNCH]);
  }
  void token_replayed() {
    if (!ev_pending) return;
    float ms = 0.f;
    if (hipEventSynchronize(ev1) == hipSuccess && hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) gpu_ms_sum += ms, gpu_tokens++;
    ev_pending = false;
  }
  void window_out(long long t0, size_t ops, size_t launches) { win_t0 = t0, win_ops = (long long)ops, win_launches = (long long)launches, win_issue_us = now_us() - t0; }
  void waited() {  // the queue has been waited for
    if (tm[TM_SYNC_OUT] < tm[TM_SYNC_IN]) tm[TM_SYNC_OUT] = now_us();
    if (win_t0 && win_ops >= 64) {  // a window went out: where an evaluation that is not replayed spends its time
      fprintf(stderr, "route timing: window of %lld ops -> %lld launches: first op handed over %.1f us before the flush, issued in %.1f us, queue empty %.1f us after the flush began\n",
              win_ops, win_launches, double(win_t0 - tm[TM_FIRST_OP]), double(win_issue_us), double(now_us() - win_t0));
      win_t0 = 0;
    }
  }
  void mark(int what, bool trace_empty) {  // ns_device.hip (bestla_device_sync / _memcpy_sync) marks a token's synchronisation (0) and the end of a copy (1)
    const long long now = now_us();
    if (what == 0) {
      if (!tm[TM_SYNC_IN] || tm[TM_SYNC_IN] < tm[TM_LAST_LAUNCH]) tm[TM_SYNC_IN] = now;
    } else if (what == 1) {  // a copy has completed: if it ended a replayed token, the token's marks are summed
      if (replayed && trace_empty && tm[TM_PREV_END] && tm[TM_FIRST_OP] > tm[TM_PREV_END] && tm[TM_SYNC_OUT] >= tm[TM_SYNC_IN]) {
        const long long m[TM_N + 1] = {tm[TM_PREV_END], tm[TM_FIRST_OP], tm[TM_FIRST_LAUNCH], tm[TM_LAST_LAUNCH], tm[TM_SYNC_IN], tm[TM_SYNC_OUT], now};
        bool ordered = true;
        for (int i = 0; i < TM_N; i++) ordered = ordered && m[i + 1] >= m[i];
        if (ordered) {
          for (int i = 0; i < TM_N; i++) tm_sum[i] += double(m[i + 1] - m[i]);
          tm_tokens++;
        }
        replayed = false;
      }
      if (trace_empty && prev_pending) tm[TM_PREV_END] = now, prev_pending = false;
    }
  }
  void report() const {
    if (gpu_tokens)
      fprintf(stderr, "route timing: %lld replayed tokens, GPU span first segment -> last %.1f us per token, host first launch -> last launch %.1f us\n", gpu_tokens,
              1e3 * gpu_ms_sum / gpu_tokens, host_us_sum / gpu_tokens);
    if (tm_tokens)
      fprintf(stderr, "route timing: per replayed token (%lld): previous token's end -> first op handed over %.1f us (the reference samples, looks the embedding up, "
                      "builds its graph) | -> first segment launched %.1f | -> last segment launched %.1f | -> the token's synchronisation entered %.1f | "
                      "-> returned (GPU finishing) %.1f | -> logits copied, token ended %.1f\n",
              tm_tokens, tm_sum[0] / tm_tokens, tm_sum[1] / tm_tokens, tm_sum[2] / tm_tokens, tm_sum[3] / tm_tokens, tm_sum[4] / tm_tokens, tm_sum[5] / tm_tokens);
  }
  void release() {
    if (ev0) (void)hipEventDestroy(ev0), (void)hipEventDestroy(ev1);
  }
};
struct Route {
  hipStream_t st = nullptr;
  bool off = false;  // this queue's graphs could not be captured (three times): plans stay off for it
  std::vector<RouteOp> cur, prev;
  size_t launched = 0;  // ops of `cur` that are on the stream already (through replayed segments or a flushed window); the rest is the window
  bool have_plan = false;
  std::vector<PlanOp> plan;
  std::vector<Segment> segs;
  std::vector<ExecOp> xops;
  int* kdev = nullptr;
  long long khost = 0;  // tokens handed to the plan (the one being verified included)
  long long kdone = 0;  // ... of which completed on it
  int pos = 0, seg = 0;
  // The reference's device pool is a bump allocator that its graph builder rewinds per layer but not per token
  // (ne_new_device_tensor_impl, ne_layers.c:904-945; llama.cpp ne_buffer_save / _load): every activation tensor of token t + 1 sits
  // a constant number of bytes above its twin of token t (4864 on the small test model).  Nothing but the token's own launches and
  // the two copies at its ends (embeddings in, logits out) ever touches those tensors, so a replayed token runs on the PLAN's
  // activations: an incoming pointer is expected at plan address + act_delta * k, the graphs use the plan addresses, and the two
  // copies are redirected there (route_translate_*).  Weights and the kv cache do not move and are compared as they are.
  long long act_delta = 0;
  std::unordered_set<const void*> act_ptrs;  // plan addresses of the shifted pointers
  bool last_replayed = false;  // the token that just ended ran from the plan: its logits are at the plan's address
  RouteTiming tmg;
  LinkPlan lp;                     // carried norms and fp16 shadows of the plan (offsets into link_mem), the RoPE angle table of XK_QKV_ROPE launches
  char* link_mem = nullptr;        // device memory behind them
  int failures = 0;  // plans that could not be captured: after a few the layer turns itself off for this queue
  // fall-backs in a row: a server alternating contexts or a beam switch makes two agreeing tokens, a plan (a capture + instantiation
  // of ~200 launches, milliseconds), and drops it on the third — from the second fall-back in a row on the next plan waits 4, 8 .. 64 agreeing tokens
  // (eight replayed tokens in a row clear the count)
  int bails_in_a_row = 0, plan_pause = 0;
  // the evaluation's inputs (see Stash): [0, stash_used) of stash_mem
  std::vector<Stash> stash;
  char* stash_mem = nullptr;
  size_t stash_cap = 0, stash_used = 0;
  bool stash_complete = true;  // false: an input of the evaluation could not be kept (it cannot be issued again from its start)
  bool stash_stale = false;    // the stash belongs to an evaluation that has ended: the next input copy starts it over — NOTHING ELSE (round 7)
  bool stash_ended = false;    // ... and that evaluation is the one that ended LAST (it brought its inputs through the queue): it can be run again from them
  bool tainted = false;        // device memory was freed while this evaluation's trace was open: the trace makes no plan and is not kept
  int copies_pending = 0;      // copies issued on the queue since it was last waited for (a wait with none pending can be left to the next copy: route_defer_sync)
  uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // tokens replayed, tokens eager, plans built, bail-outs, ops per token, captured launches per token, capture failures, -
};
std::vector<Route*> g_routes;        // one per device queue (a handful at most)
thread_local Route* t_R = nullptr;   // the queue the calling thread is serving: set by every entry that takes a stream
#define R (*t_R)
uint64_t g_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // sums over every route this process had (ns_hip_route_stats)
std::atomic<int> g_enabled{-1};        // NS_DEVICE_REPLAY / ns_hip_route_set_enabled
std::atomic<int> g_links_enabled{-1};  // NS_ROUTE_LINKS / ns_hip_route_set_enabled(3 / 5)
inline void stat(int i, uint64_t v = 1) { R.stats[i] += v, g_stats[i] += v; }
inline void stat_set(int i, uint64_t v) { R.stats[i] = v, g_stats[i] = v; }

Route* find_route(void* stream) {
  for (Route* r : g_routes)
    if (r->st == static_cast<hipStream_t>(stream)) return r;
  return nullptr;
}
// every switch of the route the environment sets, read once (the per-call part: knobs() below)
const RouteKnobs& env_knobs() {
  static const RouteKnobs env = [] {
    RouteKnobs k;
    auto off = [](const char* name) { return getenv(name) && atoi(getenv(name)) == 0; };
    auto count = [](const char* name, int dflt) {
      const int v = getenv(name) ? atoi(getenv(name)) : dflt;
      return v > 0 ? v : dflt;
    };
    k.fuse = !off("NS_ROUTE_FUSE"), k.rope_append = !off("NS_ROUTE_ROPE_APPEND"), k.qkv_rope = !off("NS_ROUTE_QKV_ROPE"), k.prefill_fuse = !off("NS_ROUTE_PREFILL_FUSE");
    k.links_env = !off("NS_ROUTE_LINKS");
    k.seg = count("NS_ROUTE_SEG", 64), k.seg0 = count("NS_ROUTE_SEG0", 16);
    k.replay = !off("NS_DEVICE_REPLAY");
    k.window = k.replay && !off("NS_ROUTE_WINDOW");
    k.lazy_sync = !off("NS_ROUTE_LAZY_SYNC");
    k.timing = getenv("NS_ROUTE_TIMING") != nullptr, k.debug = getenv("NS_ROUTE_DEBUG") != nullptr;
    k.dump = getenv("NS_ROUTE_DUMP") ? atoi(getenv("NS_ROUTE_DUMP")) : 0;
    return k;
  }();
  return env;
}
bool route_timing() { return env_knobs().timing; }
bool route_debug() { return env_knobs().debug; }
// the three switches ns_hip_route_set_enabled moves while the process runs: -1 = what the environment says
bool replay_on() {
  const int v = g_enabled.load();
  return v < 0 ? env_knobs().replay : v != 0;
}
bool enabled() { return replay_on() && !R.off; }
std::atomic<int> g_window{-1};  // NS_ROUTE_WINDOW / ns_hip_route_set_enabled
// the window: an op that is not replayed waits for the evaluation's next synchronisation point and goes out fused.  NS_ROUTE_WINDOW=0 (or the whole layer
// off: NS_DEVICE_REPLAY=0, ns_hip_route_set_enabled(0)): it launches when it is handed over, one launch per operator (round 5 / round 4)
bool window_on() {
  const int v = g_window.load();
  return v < 0 ? env_knobs().window : v != 0;
}
// carried norms: on by default (NS_ROUTE_LINKS=0 or ns_hip_route_set_enabled(5) turn them off, (3) forces them on; ns_route_fuse.cpp link_norms)
bool links_on() {
  const int v = g_links_enabled.load();
  return v < 0 ? env_knobs().links_env : v != 0;
}
RouteKnobs knobs() {
  RouteKnobs k = env_knobs();
  k.kv16 = kv16_enabled(), k.links = links_on();
  return k;
}
// the planner's questions about the device, answered for one queue
struct DeviceEnv : RouteEnv {
  hipStream_t st;
  explicit DeviceEnv(hipStream_t s) : st(s) {}
  bool mirror_of_cell(const void* cell, KvMirrorArgs* out) override { return kvm_args_for_cell(cell, out); }
  bool mirror_for_producer(const void* k32, const void* v32, int heads_kv, int hs, int n_ctx, int n_past, int m, _Float16** k16, _Float16** v16) override {
    return kvm_for_producer(k32, v32, heads_kv, hs, n_ctx, n_past, m, k16, v16);
  }
  void* scratch(size_t bytes, int slot) override { return stream_scratch(st, bytes, slot); }
  bool weight_carries_norm(const ns_weight* w) override { return route_link_weight_ok(w); }
};

// the kv mirrors a plan's cache writes kept current (ns_route.h): positions below the context length of the last COMPLETED token hold the cache
void mark_mirrors() {
  if (!R.have_plan) return;
  for (const PlanOp& po : R.plan)
    if (po.op.kind == RK_MHA) kvm_set_valid(MhaView{po.op}.k(), int(MhaView{po.op}.seq_all() + (po.moving == 1 ? po.delta : 0) * R.kdone));
}
// the plan's link memory and what describes it
void release_links() {
  R.lp = LinkPlan{};
  if (R.link_mem) (void)hipFree(R.link_mem), R.link_mem = nullptr;
}
void drop_plan() {
  mark_mirrors();
  // graphs that may still be running are not destroyed under them (only hipFree(link_mem) synchronised, and only with links)
  if (!R.segs.empty() && R.st) (void)hipStreamSynchronize(R.st);
  for (Segment& s : R.segs)
    if (s.exec) (void)hipGraphExecDestroy(s.exec);
  R.segs.clear();
  R.xops.clear();
  release_links();
  R.plan.clear();
  R.have_plan = false;
  R.pos = R.seg = 0;
  R.khost = R.kdone = 0;
  R.act_delta = 0;
  R.act_ptrs.clear();
  R.last_replayed = false;
}

// plan op j as token k of the plan would hand it over
RouteOp expected(const PlanOp& po, long long k) {
  RouteOp e = po.op;
  if (po.moving == 1) e.i[moving_int(e.kind)] += po.delta * k;
  if (po.moving == 2) e.p[moving_ptr(e.kind)] = static_cast<const char*>(e.p[moving_ptr(e.kind)]) + po.delta * k;
  for (int x = 0; x < 4; x++)
    if (po.pshift & (1u << x)) e.p[x] = static_cast<const char*>(e.p[x]) + R.act_delta * k;
  return e;
}

// The evaluation's inputs are put back where the graph asked for them (Stash): segments of a plan run on the PLAN's activations, and a
// token's own tensors sit only act_delta * k above those — inside memory the segments have written.
// `ended`: the evaluation has ended (route_after_sync runs it again) — its stash is stale by then, which only says that the NEXT input copy starts it over;
// whether it holds that evaluation's inputs is stash_ended.  Round 6 asked stash_stale in both places and restored nothing behind an evaluation's end: a
// REPLAYED token that was run again (fp16 overflow) read an input the plan's segments had written over.
int restore_inputs(bool ended = false) {
  if (ended ? !R.stash_ended : R.stash_stale) return 0;  // (this evaluation brought no input through the queue)
  for (const Stash& si : R.stash)
    if (hipMemcpyAsync(si.dst, R.stash_mem + si.off, si.bytes, hipMemcpyDeviceToDevice, R.st) != hipSuccess) {
      set_error("device route: restoring an evaluation's input failed");
      return -1;
    }
  return 0;
}
// The token deviates from the plan.  Segments launched so far ran on the PLAN's activations, the reference's remaining launches will read
// the addresses it asked for: the token is issued again from its first launch at those addresses — its verified ops are in R.cur, every
// launch of the route is a pure function of its inputs, kv-cache cells are rewritten with the same values, and the token's input is put back
// from its stash.  "Issued" = left to the window (R.launched says from where); the plan is forgotten.
int bail_out() {
  stat(3);
  int rc = 0;
  if (R.act_delta != 0) {
    if (R.seg > 0) rc = restore_inputs();
    R.launched = 0;
  } else {
    R.launched = size_t(R.seg < int(R.segs.size()) ? R.segs[R.seg].beg : R.pos);
  }
  R.bails_in_a_row = std::min(R.bails_in_a_row + 1, 6);
  R.plan_pause = R.bails_in_a_row >= 2 ? 1 << R.bails_in_a_row : 0;  // (one fall-back — a new prompt — costs nothing: the next two agreeing tokens make a plan)
  drop_plan();
  return rc;
}

void explain_mismatch(size_t j, const RouteOp& a, const RouteOp& b) {
  fprintf(stderr, "route: op %zu (kind %u vs %u) differs between consecutive tokens in more than its moving value:", j, a.kind, b.kind);
  for (int x = 0; x < 4; x++)
    if (a.p[x] != b.p[x]) fprintf(stderr, " p[%d] %p -> %p (%+lld)", x, a.p[x], b.p[x], (long long)(static_cast<const char*>(b.p[x]) - static_cast<const char*>(a.p[x])));
  for (int x = 0; x < 24; x++)
    if (a.i[x] != b.i[x]) fprintf(stderr, " i[%d] %lld -> %lld", x, a.i[x], b.i[x]);
  for (int x = 0; x < 8; x++)
    if (memcmp(&a.f[x], &b.f[x], 4)) fprintf(stderr, " f[%d] %g -> %g", x, a.f[x], b.f[x]);
  fprintf(stderr, "\n");
}

// ---- making a plan from two consecutive agreeing tokens ----
// what a plan needs on the device before anything is captured: the token counter at 0, the scratch of the moving-length attention
bool prepare_plan_device(const std::vector<PlanOp>& plan) {
  if (!R.kdev && hipMalloc(reinterpret_cast<void**>(&R.kdev), 64) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (hipMemsetAsync(R.kdev, 0, 64, R.st) != hipSuccess || hipStreamSynchronize(R.st) != hipSuccess) return false;
  // scratch the moving-length attention needs (partials laid out for the longest context): sized BEFORE any capture
  for (const PlanOp& po : plan)
    if (po.op.kind == RK_MHA) {
      const MhaView a{po.op};
      if (!stream_scratch(R.st, mha_f32_partials_bytes(int(a.batch()), int(a.seq()), int(a.heads()), int(a.head_size()), int(a.n_ctx())), SLOT_MHA_PARTIALS)) return false;
      if (!stream_scratch_zeroed(R.st, kMhaTicketBytes, SLOT_MHA_TICKETS)) return false;  // the tickets of the merge inside the launch (ns_device_mha.hip)
      // ... and what the fp16-mirror form needs (ns_attn.cpp, moving context length)
      if (kv16_enabled() && !attn_prepare_moving(R.st, int(a.batch()), int(a.heads()), int(a.heads_kv()), int(a.head_size()), int(a.n_ctx()))) return false;
    }
  return true;
}
// every segment's launches into a HIP graph of its own; the first one also moves the token counter
bool capture_segments(const std::vector<ExecOp>& xops, const std::vector<PlanOp>& plan, std::vector<Segment>& segs) {
  const LinkMem lm{R.link_mem, &R.lp};
  bool ok = true;
  for (size_t sg = 0; sg < segs.size() && ok; sg++) {
    hipGraph_t graph = nullptr;
    if (hipStreamBeginCapture(R.st, hipStreamCaptureModeRelaxed) != hipSuccess) return false;
    if (sg == 0) hipLaunchKernelGGL(route_count_kernel, dim3(1), dim3(1), 0, R.st, R.kdev);
    for (int e = segs[sg].xbeg; e < segs[sg].xend && ok; e++) ok = issue_launch(xops[e], plan, lm, R.kdev, R.st) == 0;
    ok = flush_lazy_node() == 0 && ok;
    const hipError_t ec = hipStreamEndCapture(R.st, &graph);
    ok = ok && ec == hipSuccess && graph != nullptr;
    if (ok) ok = hipGraphInstantiate(&segs[sg].exec, graph, nullptr, nullptr, 0) == hipSuccess;
    if (graph) (void)hipGraphDestroy(graph);
  }
  return ok;
}
// one attempt at a plan's graphs: the launches (fused where possible), their segments, the captures
bool attempt_capture(const std::vector<PlanOp>& plan, const RouteKnobs& kn, bool with_links, std::vector<ExecOp>& xops, std::vector<Segment>& segs) {
  DeviceEnv env(R.st);
  release_links();
  xops = plan_launches(plan, kn, env, with_links, &R.lp);
  if (R.lp.bytes && hipMalloc(reinterpret_cast<void**>(&R.link_mem), R.lp.bytes) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  segs.clear();
  for (const SegmentCut& c : cut_segments(xops, plan, kn)) {
    Segment s;
    static_cast<SegmentCut&>(s) = c;
    segs.push_back(s);
  }
  if (segs.empty()) return false;
  if (capture_segments(xops, plan, segs)) return true;
  if (kn.debug) fprintf(stderr, "route: capture %s failed: %s\n", with_links ? "with carried norms" : "", ns_hip_last_error());
  (void)hipGetLastError();
  ns_hip_reset_error();
  for (Segment& sg : segs)
    if (sg.exec) (void)hipGraphExecDestroy(sg.exec), sg.exec = nullptr;
  return false;
}
void dump_plan(const std::vector<PlanOp>& plan, int lim) {  // NS_ROUTE_DUMP
  static const char* names[] = {"?", "GEMM", "ADD", "MUL", "SILU", "RMSNORM", "ROPE", "ROPE_YARN", "DUP", "MHA"};
  for (size_t j = 0; j < plan.size() && int(j) < lim; j++) {
    const RouteOp& o = plan[j].op;
    fprintf(stderr, "route plan %3zu %-8s p %p %p %p %p  i %lld %lld %lld %lld %lld  shift %x moving %d delta %lld\n", j, names[o.kind < 10 ? o.kind : 0],
            o.p[0], o.p[1], o.p[2], o.p[3], o.i[0], o.i[1], o.i[2], o.i[3], o.i[4], plan[j].pshift, plan[j].moving, plan[j].delta);
  }
}
bool make_plan() {
  const RouteKnobs kn = knobs();
  if (kn.debug) fprintf(stderr, "route: token ended with %zu ops (previous token: %zu)\n", R.cur.size(), R.prev.size());
  DeviceEnv env(R.st);
  TokenPlan tp;
  const NoPlan no = diff_tokens(R.prev, R.cur, env, &tp);
  if (no.why) {
    if (kn.debug && no.differs) explain_mismatch(size_t(no.at), R.prev[no.at], R.cur[no.at]);
    if (kn.debug) fprintf(stderr, "route: no plan (%s, op %ld)\n", no.why, no.at);
    return false;
  }
  if (!prepare_plan_device(tp.ops)) return false;
  // with carried norms first; should their captures be refused (a weight or shape the decode kernel does not carry a norm for), once more without them
  std::vector<ExecOp> xops;
  std::vector<Segment> segs;
  if (!(links_wanted(kn) && attempt_capture(tp.ops, kn, true, xops, segs)) && !attempt_capture(tp.ops, kn, false, xops, segs)) {
    release_links();
    stat(6);
    if (++R.failures >= 3) {  // this queue's graphs cannot be captured: its evaluations stay on the window
      R.off = true;
      fprintf(stderr, "ns route: the per-token graph of device queue %p could not be captured %d times (%s): replay is off for this queue, "
                      "its evaluations keep running as fused launches\n", (void*)R.st, R.failures, ns_hip_last_error());
    }
    return false;
  }
  dump_plan(tp.ops, kn.dump);
  const size_t n = tp.ops.size();
  R.plan.swap(tp.ops);
  R.segs.swap(segs);
  stat_set(5, xops.size());
  R.xops.swap(xops);
  R.act_delta = tp.act_delta;
  R.act_ptrs.swap(tp.act_ptrs);
  R.last_replayed = false;
  R.have_plan = true;
  R.khost = R.kdone = 0;
  R.pos = R.seg = 0;
  stat(2);
  stat_set(4, n);
  return true;
}

// ---- the window: ops handed over and not launched yet, cur[launched ..) ----
// They go out at the next synchronisation point of the queue, as the fused launches the planner finds among them.  `src` / `bytes`: the copy that
// ends the window reads this (a fusion then keeps the tensor it would have left out).
int flush_window(const void* src, size_t bytes) {
  if (R.launched >= R.cur.size()) return 0;
  std::vector<PlanOp> w(R.cur.size() - R.launched);
  for (size_t j = 0; j < w.size(); j++) w[j] = PlanOp{R.cur[R.launched + j], 0, 0, 0u};
  const long long t0 = route_timing() ? now_us() : 0;
  DeviceEnv env(R.st);
  std::vector<ExecOp> x = window_launches(w, knobs(), env, ExtraRead{static_cast<const char*>(src), bytes});
  int rc = 0;
  for (size_t e = 0; e < x.size() && rc == 0; e++) {
    rc = issue_launch(x[e], w, LinkMem{}, nullptr, R.st);
    // an attention that took the fp32 kernels left no fp16 rows behind: the projection that was promised them converts its own
    if (rc == 0 && x[e].o16p && x[e].xk == XK_OP && w[x[e].idx[0]].op.kind == RK_MHA && !g_mha_out16_written)
      for (size_t c = e + 1; c < x.size(); c++)
        if (x[c].a16p == x[e].o16p) x[c].a16p = nullptr;
  }
  if (route_timing()) R.tmg.window_out(t0, w.size(), x.size());
  rc = flush_lazy_node() != 0 ? -1 : rc;
  R.launched = R.cur.size();
  if (rc != 0) fprintf(stderr, "Err: invalid parameters (device route: %s)\n", ns_hip_last_error());
  return rc;
}
constexpr size_t kWindowMax = 16384;  // ops; a window this long goes out without waiting for a synchronisation (no model graph comes near)

// an evaluation that ended is evaluated AGAIN from its first launch, plainly (no plan, the fp32 kernels): R.cur holds its ops, the stash its inputs
int reevaluate() {
  if (!R.stash_complete || R.cur.empty()) return -1;
  if (restore_inputs(true) != 0) return -1;
  R.launched = 0;
  return flush_window(nullptr, 0);
}

}  // namespace

void route_attach(void* stream) {
  if (find_route(stream)) return;
  Route* r = new Route();
  r->st = static_cast<hipStream_t>(stream);
  g_routes.push_back(r);
}
void route_detach(void* stream) {
  Route* r = find_route(stream);
  if (!r) return;
  t_R = r;
  if (route_timing()) R.tmg.report();
  drop_plan();
  if (R.stash_mem) (void)hipFree(R.stash_mem);
  if (R.kdev) (void)hipFree(R.kdev);
  R.tmg.release();
  g_routes.erase(std::find(g_routes.begin(), g_routes.end(), r));
  delete r;
  t_R = nullptr;
}
bool route_hook(void* stream) {
  if (route_executing()) return false;
  Route* r = find_route(stream);
  if (!r) return false;
  t_R = r;
  return window_on() || enabled();
}

int route_submit(const RouteOp& op) {
  if (route_timing() && R.cur.empty()) R.tmg.first_op();
  if (R.have_plan) {
    if (R.pos == 0) R.khost++, R.last_replayed = false;
    if (R.pos < int(R.plan.size())) {
      const RouteOp e = expected(R.plan[R.pos], R.khost);
      if (memcmp(&e, &op, sizeof(RouteOp)) == 0) {
        R.cur.push_back(op);
        R.pos++;
        if (R.pos == R.segs[R.seg].end) {
          if (route_timing() && R.seg == 0) R.tmg.first_segment(R.st);
          if (hipGraphLaunch(R.segs[R.seg].exec, R.st) != hipSuccess) {
            set_error("device route: launching a replayed segment failed");
            return -1;
          }
          R.seg++;
          R.launched = size_t(R.pos);
          if (route_timing() && R.seg == int(R.segs.size())) R.tmg.last_segment(R.st);
        }
        return 0;
      }
    }
    if (route_debug()) {
      fprintf(stderr, "route: token %lld of the plan deviates at launch %d of %zu\n", R.khost, R.pos, R.plan.size());
      if (R.pos < int(R.plan.size())) explain_mismatch(size_t(R.pos), expected(R.plan[R.pos], R.khost), op);
    }
    if (bail_out() != 0) return -1;  // (this op is not in R.cur yet)
  }
  R.cur.push_back(op);
  if (!window_on()) {  // round-5 behaviour: launched as it comes
    R.launched = R.cur.size();
    return execute(op, R.st);
  }
  return R.cur.size() - R.launched >= kWindowMax ? flush_window(nullptr, 0) : 0;
}

// a synchronisation point of the route's stream: everything handed over so far must be on the stream; a non-empty trace ends a token.
// `src` / `bytes`: the device-side source of the copy that follows (nullptr: a plain synchronisation)
int route_sync_point(void* stream, const void* src, size_t bytes) {
  if (route_executing()) return 0;
  Route* r = find_route(stream);
  if (!r) return 0;
  t_R = r;
  if (!window_on() && !enabled()) return 0;
  int rc = 0;
  if (R.have_plan) {
    if (R.pos == int(R.plan.size())) {  // the whole token matched: every segment is on the stream
      stat(0);
      R.kdone = R.khost;
      R.pos = R.seg = 0;
      R.launched = 0;
      R.prev.swap(R.cur);
      R.cur.clear();
      R.last_replayed = true;
      R.tmg.replayed = true;
      R.stash_ended = !R.stash_stale;
      R.stash_stale = R.tmg.prev_pending = true;
      if (R.bails_in_a_row && R.kdone >= 8) R.bails_in_a_row = 0;
      R.tmg.token_replayed();
      return 0;
    }
    if (R.pos > 0) rc = bail_out();  // the token ended (or synchronised) inside the plan
  }
  if (!R.cur.empty()) {
    if (flush_window(src, bytes) != 0) rc = -1;
    // the evaluation ends here (its trace is complete): a plan is made from two consecutive agreeing ones
    stat(1);
    if (!R.have_plan && rc == 0 && enabled() && !R.tainted) {
      if (R.plan_pause > 0 && R.cur.size() == R.prev.size()) R.plan_pause--;
      else if (R.plan_pause == 0) (void)make_plan();
    }
    R.prev.swap(R.cur);
    R.cur.clear();
    if (R.tainted) R.prev.clear(), R.tainted = false;  // (a free inside the evaluation: its ops may name memory that is gone)
    R.launched = 0;
    R.stash_ended = !R.stash_stale;
    R.stash_stale = R.tmg.prev_pending = true;
  }
  return rc;
}

// bestla_device_sync has waited for the queue: the end of an evaluation.  A value that did not fit fp16 in one of the route's fp16 shortcuts (the kv
// mirror, a carried norm's shadow) raised the flag: the shortcuts are turned off for the process and the evaluation that just ended — its ops are in
// `prev`, its inputs in the stash — is evaluated again on the fp32 forms before anybody reads its results.
bool route_after_sync(void* stream) {
  if (route_executing()) return false;
  Route* r = find_route(stream);
  if (!r) return false;
  t_R = r;
  R.copies_pending = 0;
  if (route_timing()) R.tmg.waited();
  if (!kvm_overflowed()) return false;
  kvm_overflow_reset();
  const bool had_f16 = kv16_enabled() || links_on();
  kv16_set(0);
  g_links_enabled.store(0);
  if (!had_f16) return false;
  bool again = false;
  fprintf(stderr, "ns route: a value beyond the fp16 range (|x| > 65504) met an fp16 shortcut of the device route (the kv mirror or a carried norm's "
                  "shadow): both are off for this process from here on (the fp32 kernels of the reference's device path take over), the evaluation is run again\n");
  for (Route* q : g_routes) {
    t_R = q;
    const bool mine = q == r && !q->prev.empty() && q->cur.empty();
    drop_plan();
    if (mine) {
      R.cur.swap(R.prev);  // the evaluation that just ended
      const int rc = reevaluate();
      R.prev.swap(R.cur);
      R.cur.clear();
      R.launched = 0;
      if (rc != 0) fprintf(stderr, "ns route: the evaluation could not be run again (%s): its results hold the overflow (inf / nan)\n", ns_hip_last_error());
      (void)hipStreamSynchronize(R.st);
      kvm_overflow_reset();
      again = rc == 0;
    }
  }
  t_R = r;
  return again;
}
// bestla_device_sync with nothing but launches on the queue since it was last waited for: nothing the host can see depends on them before a copy
// is asked for — and that copy is ordered behind them on the queue.  The reference's evaluation ends with sync, copy, sync (ne_layers.c:8345-8346): the
// first of the two waits is left to the second.  For a token this measured level (2074 vs 2065 / 2088 us at 1500 cached positions).  For a prompt it is
// what lets the copy's host-side preparation run UNDER the launches instead of behind them: the copy of a 1500-token prompt's logits (192 MB into pages
// the reference has not touched yet) arrives while the queue still has 28 ms of work, the runtime maps the destination and ns_device.hip first-touches
// it meanwhile — first evaluation of a process 59.0 -> 52.1 (deferral alone) -> 46.2 / 48.4 ms on one box (profiles/r06_route_timings.txt), later
// evaluations unchanged.  NS_ROUTE_LAZY_SYNC=0 waits where the caller asked.
bool route_defer_sync(void* stream) {
  if (!env_knobs().lazy_sync || route_executing()) return false;
  Route* r = find_route(stream);
  return r && r->copies_pending == 0 && (window_on() || replay_on());
}
void route_note_copy(void* stream) {
  Route* r = find_route(stream);
  if (r) r->copies_pending++;
}
void route_time_mark(void* stream, int what) {  // NS_ROUTE_TIMING: ns_device.hip marks a token's synchronisation and its end
  if (!route_timing() || route_executing()) return;
  Route* r = find_route(stream);
  if (r) r->tmg.mark(what, r->cur.empty());
}

// bestla_device_memcpy on the route's queue while a plan is held.  The copy that brings a token's embeddings has an activation of the NEXT
// token as its destination (expected at plan address + act_delta * (k + 1)): the bytes go where they were asked for AND to the plan's twin of
// that tensor (returned here; nullptr: no twin), so a token that is replayed finds them and a token that falls back does too.  The copy that
// fetches a replayed token's logits reads the plan's address.  Pointers that are not the plan's activations pass through.
void* route_twin_dst(void* dst, void* stream) {
  Route* r = find_route(stream);
  if (route_executing() || !r || !r->have_plan || r->act_delta == 0 || r->pos != 0) return nullptr;
  void* cand = static_cast<char*>(dst) - r->act_delta * (r->khost + 1);
  return r->act_ptrs.count(cand) ? cand : nullptr;
}
const void* route_translate_src(const void* src, void* stream) {
  Route* r = find_route(stream);
  if (route_executing() || !r || !r->have_plan || r->act_delta == 0 || !r->last_replayed) return src;
  const void* cand = static_cast<const char*>(src) - r->act_delta * r->khost;
  return r->act_ptrs.count(cand) ? cand : src;
}
// a copy INTO device memory on the route's queue has been issued.  In front of an evaluation's first op it brings an input of that evaluation:
// a device-side copy is kept (D2D behind it on the queue) so that the evaluation can be issued again from its start (bail_out, route_after_sync).
void route_note_input(void* dst, size_t bytes, void* stream) {
  Route* r = find_route(stream);
  if (route_executing() || !r || !dst || !bytes) return;
  t_R = r;
  if (!R.cur.empty() || R.pos != 0) return;  // (cannot happen: a copy is a synchronisation point, which ends the trace)
  if (R.stash_stale) R.stash.clear(), R.stash_used = 0, R.stash_complete = true, R.stash_stale = R.stash_ended = false;
  constexpr size_t kStashMax = size_t(64) << 20;
  if (bytes > kStashMax) return;  // (a model part being uploaded, not an evaluation's input: nothing an evaluation writes over)
  // The stash keeps what arrives directly IN FRONT of an evaluation.  Copies that together pass the largest single input it keeps are a load as well (the
  // reference's loader copies tensor by tensor, model_files.h:1523; a session's caches): what is kept so far is let go and the stash starts over with this
  // copy — an evaluation writes over its activations, which the copies directly in front of it fill, not over weights or cache rows it does not rewrite with
  // the same values.  (Round 6 kept everything since the process began in a buffer that doubled, gave up once that asked for more than 512 MB and left a
  // first evaluation that overflowed with its inf / nan.)
  if (((R.stash_used + 255) & ~size_t(255)) + bytes > kStashMax) R.stash.clear(), R.stash_used = 0, R.stash_complete = true;
  const size_t need = ((R.stash_used + 255) & ~size_t(255)) + bytes;
  if (need > R.stash_cap) {  // grows; what this evaluation has kept so far moves along
    char* bigger = nullptr;
    const size_t want = std::max<size_t>(need * 2, size_t(1) << 20);
    if (want > (size_t(512) << 20) || hipMalloc(reinterpret_cast<void**>(&bigger), want) != hipSuccess) {
      (void)hipGetLastError();
      R.stash_complete = false;
      return;
    }
    if (R.stash_used) (void)hipMemcpyAsync(bigger, R.stash_mem, R.stash_used, hipMemcpyDeviceToDevice, R.st);
    (void)hipStreamSynchronize(R.st);
    if (R.stash_mem) (void)hipFree(R.stash_mem);
    R.stash_mem = bigger, R.stash_cap = want;
  }
  const size_t off = (R.stash_used + 255) & ~size_t(255);
  if (off + bytes > R.stash_cap || hipMemcpyAsync(R.stash_mem + off, dst, bytes, hipMemcpyDeviceToDevice, R.st) != hipSuccess) {
    (void)hipGetLastError();
    R.stash_complete = false;
    return;
  }
  R.stash.push_back(Stash{dst, bytes, off});
  R.stash_used = off + bytes;
}
// device memory is being freed: no captured launch, no recorded op may outlive it — and none may be LOST (round 7: round 6 cleared the window with its ops
// not launched yet, and dropped the plan under a token whose first segments had run on the plan's activations).  What has been handed over goes out first:
// a token under verification falls back (it is issued again at the addresses it asked for, as when it deviates), the window is flushed.  The open trace
// stays — the evaluation goes on behind the free and ends as one evaluation — but makes no plan and is not kept for the next one.
void route_invalidate() {
  if (route_executing()) return;
  Route* keep = t_R;
  for (Route* r : g_routes) {
    t_R = r;
    if (R.have_plan && R.pos > 0) (void)bail_out();
    if (!R.cur.empty()) {
      (void)flush_window(nullptr, 0);
      R.tainted = true;
    }
    drop_plan();
    R.prev.clear();
    R.stash_ended = false;  // (`prev` is gone: nothing to run again)
  }
  t_R = keep;
}

}  // namespace ns

extern "C" void ns_hip_route_stats(uint64_t out[8]) {
  for (int i = 0; i < 8; i++) out[i] = ns::g_stats[i];
  out[7] = 0;
  for (const ns::Route* r : ns::g_routes) out[7] |= r->have_plan ? 1 : 0;
}
extern "C" int ns_hip_route_set_enabled(int on) {
  const int prev = ns::replay_on() ? 1 : 0;
  // 0: the layer is off (every op launches when it is handed over); 1: window + plans (3: with carried norms, 5: without, 1: NS_ROUTE_LINKS, default on);
  // 8: the window alone (evaluations go out fused, no plan is made)
  if (!(on & 1)) ns::route_invalidate();
  ns::g_enabled.store((on & 1) ? 1 : 0);
  ns::g_window.store(on ? 1 : 0);
  if (on & 1) ns::g_links_enabled.store((on & 2) ? 1 : (on & 4) ? 0 : -1);
  for (ns::Route* r : ns::g_routes) r->failures = 0, r->off = false, r->bails_in_a_row = r->plan_pause = 0;
  return prev;
}
