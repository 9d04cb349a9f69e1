// Launch-list executor: one C-ABI call issues a whole segment of a plan's prepared launches on the streams of the train step.
//
// A plan (kurosiwo_amd/*_plan.py) is a flat list of prepared entry-point calls plus ordering entries; until round 5 the host walked it in
// Python -- one ctypes call, one torch stream switch and up to three torch event calls per launch: 9 ms of host time for the ~290
// launches of an SNUNet step, 29 ms for ChangeFormer's ~730 (bench `host_issue_ms_per_step`), i.e. the step was about to become
// host-bound.  Here the list is compiled ONCE into an array of ksmi_op (function pointer, thunk of its
// signature, 64-bit argument slots, lane / side-stream tags) and ksmi_run_list replays a segment of it.  The Python walk
// (launch.LaunchList.run) stays as the timed / hooked path and as the cross-check (tests/test_gpu_graph.py holds the two to the same
// bits); it makes its launches itself but takes every cross-stream edge from the same Runner (ksmi_runner_order / _fork_side /
// _mark_side / _wait_side), so the fork / tag / busy state of a step has ONE owner and the lists of a step may mix the two walks.
//
// Streams (launch.StepStreams): main = lane 0, lane1 = second compute lane, side / side2 = weight-gradient streams.
//   CALL, plain:     launch on the stream of its lane.
//   CALL, side:      the side stream waits for an event recorded on the launch's lane stream ("fork"), the launch goes to the side
//                    stream, and a tagged launch records an event there that a later WAIT_SIDE(tag) consumes.
//   ORDER(a, b):     lane b waits for everything lane a was handed so far.
//   WAIT_SIDE(tag):  the issuing lane and the lane of the last launch wait for that tagged side-stream launch (tag < 0: for the whole
//                    side stream, if it is busy; a tag that was never recorded: nothing).
//   JOIN:            main waits for every other stream that was handed work (end of the step).
// Events come from a fixed ring created once (hipEventDisableTiming): hipStreamWaitEvent captures the record it finds when it is
// enqueued, so a ring slot may be re-recorded as soon as the wait call has returned.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <unordered_map>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/ksmi.h"
#include "errors.h"
#include "thunks_gen.h"

namespace {

constexpr int kRing = 64;

struct Runner {
  hipStream_t main = nullptr, lane1 = nullptr, side = nullptr, side2 = nullptr;
  bool lanes = false, use_side = false;
  bool dirty = false, side_busy = false;
  int cur = 0;                                   // lane of the last launch of the list being walked
  hipEvent_t ring[kRing];
  int next = 0;
  bool have_ring = false;
  std::unordered_map<int, hipEvent_t> tagged;    // side tag -> event recorded behind that launch
  std::vector<hipEvent_t> tag_pool;              // events of consumed tags, for reuse

  hipStream_t stream(int lane) const { return (lanes && lane == 1 && lane1) ? lane1 : main; }
  int ensure_ring() {
    if (have_ring) return 0;
    for (int i = 0; i < kRing; ++i)
      if (hipEventCreateWithFlags(&ring[i], hipEventDisableTiming) != hipSuccess) return ksmi_fail(KSMI_E_UNSUPPORTED, "run_list: hipEventCreate");
    have_ring = true;
    return 0;
  }
  // dst waits for everything src was handed so far
  int order(hipStream_t src, hipStream_t dst) {
    if (src == dst) return 0;
    if (int rc = ensure_ring()) return rc;              // (created at the first cross-stream edge: single-stream lists never need events)
    hipEvent_t ev = ring[next];
    next = (next + 1) % kRing;
    if (hipEventRecord(ev, src) != hipSuccess || hipStreamWaitEvent(dst, ev, 0) != hipSuccess) return ksmi_fail(KSMI_E_UNSUPPORTED, "run_list: event record / wait");
    return 0;
  }
  // ORDER(a, b): lane b waits for everything lane a was handed so far
  int order_lanes(int a, int b) {
    if (!lanes) return 0;
    if (int rc = order(stream(a), stream(b))) return rc;
    dirty = true;
    return 0;
  }
  hipStream_t side_stream(int side_ix) const { return (side_ix && side2) ? side2 : side; }
  // the side stream of a weight gradient waits for what its lane was handed so far; *out = the stream the launch goes to
  int fork_side(int lane, int side_ix, hipStream_t* out) {
    hipStream_t S = stream(lane);
    *out = S;
    if (!use_side) return 0;
    hipStream_t SS = side_stream(side_ix);
    if (int rc = order(S, SS)) return rc;
    dirty = side_busy = true;
    *out = SS;
    return 0;
  }
  // record the event of `tag` behind the side-stream launch just made
  int mark_side(int tag, int side_ix) {
    if (!use_side || tag < 0) return 0;
    hipEvent_t ev;
    auto it = tagged.find(tag);
    if (it != tagged.end()) ev = it->second;
    else {
      if (!tag_pool.empty()) { ev = tag_pool.back(); tag_pool.pop_back(); }
      else if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return ksmi_fail(KSMI_E_UNSUPPORTED, "run_list: hipEventCreate");
      tagged[tag] = ev;
    }
    if (hipEventRecord(ev, side_stream(side_ix)) != hipSuccess) return ksmi_fail(KSMI_E_UNSUPPORTED, "run_list: event record");
    return 0;
  }
  // the waiting streams: the lane the list was on when the entry was appended (lane) AND the lane of the last launch (cur_lane)
  int wait_side(int lane, int cur_lane, int tag) {
    if (!use_side) return 0;
    hipStream_t w0 = stream(lanes ? lane : 0), w1 = stream(cur_lane);
    if (tag < 0) {
      if (!side_busy) return 0;                         // (nothing handed to a side stream since the last such wait)
      for (hipStream_t SS : {side, side2}) {
        if (!SS) continue;
        int rc;
        if ((rc = order(SS, w0)) || (w1 != w0 && (rc = order(SS, w1)))) return rc;
      }
      side_busy = false;
      return 0;
    }
    auto it = tagged.find(tag);
    if (it == tagged.end()) return 0;                   // (never recorded, or consumed already)
    if (hipStreamWaitEvent(w0, it->second, 0) != hipSuccess || (w1 != w0 && hipStreamWaitEvent(w1, it->second, 0) != hipSuccess))
      return ksmi_fail(KSMI_E_UNSUPPORTED, "run_list: wait on a tagged side event");
    tag_pool.push_back(it->second);
    tagged.erase(it);
    return 0;
  }
};

}  // namespace

extern "C" {

int ksmi_thunk_id(const char* sig) {
  if (!sig) return -1;
  for (int i = 0; i < ksmi_n_thunks; ++i)
    if (!strcmp(sig, ksmi_thunk_sigs[i])) return i;
  return -1;
}

void* ksmi_runner_create(void) { return new Runner(); }

int ksmi_runner_destroy(void* r_) {
  Runner* r = (Runner*)r_;
  if (!r) return 0;
  if (r->have_ring) for (int i = 0; i < kRing; ++i) (void)hipEventDestroy(r->ring[i]);
  for (auto& kv : r->tagged) (void)hipEventDestroy(kv.second);
  for (hipEvent_t e : r->tag_pool) (void)hipEventDestroy(e);
  delete r;
  return 0;
}

int ksmi_runner_set_streams(void* r_, void* main, void* lane1, void* side, void* side2) {
  Runner* r = (Runner*)r_;
  if (!r) return ksmi_fail(KSMI_E_ARG, "runner_set_streams: null runner");
  r->main = (hipStream_t)main; r->lane1 = (hipStream_t)lane1; r->side = (hipStream_t)side; r->side2 = (hipStream_t)side2;
  r->lanes = lane1 != nullptr;
  r->use_side = side != nullptr;
  return 0;
}

int ksmi_run_list(void* r_, const ksmi_op* ops, int first, int last, const uint8_t* skip, int32_t* failed_at) {
  Runner* r = (Runner*)r_;
  if (!r || !ops || first < 0 || last < first) return ksmi_fail(KSMI_E_ARG, "run_list: bad arguments");
  if (failed_at) *failed_at = -1;
  if (first == 0) r->cur = 0;
  for (int i = first; i < last; ++i) {
    const ksmi_op& op = ops[i];
    int rc = 0;
    switch (op.kind) {
      case KSMI_OP_CALL: {
        if (skip && skip[i]) break;
        if (op.sig < 0 || op.sig >= ksmi_n_thunks || !op.fn) { rc = ksmi_fail(KSMI_E_ARG, "run_list: bad thunk / function"); break; }
        const int lane = r->lanes ? op.lane : 0;
        r->cur = lane;
        if (op.side && r->use_side) {
          hipStream_t SS;
          if ((rc = r->fork_side(lane, op.side - 1, &SS))) break;
          rc = ksmi_thunks[op.sig](op.fn, op.args, SS);
          if (rc == 0 && op.tag >= 0) rc = r->mark_side(op.tag, op.side - 1);
        } else {
          rc = ksmi_thunks[op.sig](op.fn, op.args, r->stream(lane));
        }
        break;
      }
      case KSMI_OP_ORDER:
        rc = r->order_lanes(op.a, op.b);
        break;
      case KSMI_OP_WAIT_SIDE:
        rc = r->wait_side(op.lane, r->cur, op.tag);
        break;
      default:
        rc = ksmi_fail(KSMI_E_ARG, "run_list: unknown op kind");
    }
    if (rc) { if (failed_at) *failed_at = i; return rc; }
  }
  return 0;
}

// The same four transitions for the host-language walk of a list (launch.LaunchList.run: timed runs, hooks on every entry, SyncBN's
// collectives), so that both walks of one step share one fork / tag / busy state.
int ksmi_runner_order(void* r_, int src_lane, int dst_lane) {
  Runner* r = (Runner*)r_;
  if (!r) return ksmi_fail(KSMI_E_ARG, "runner_order: null runner");
  return r->order_lanes(src_lane, dst_lane);
}

int ksmi_runner_fork_side(void* r_, int lane, int side_ix, void** stream_out) {
  Runner* r = (Runner*)r_;
  if (!r || !stream_out) return ksmi_fail(KSMI_E_ARG, "runner_fork_side: null runner / stream_out");
  hipStream_t SS = nullptr;
  int rc = r->fork_side(lane, side_ix, &SS);
  *stream_out = (void*)SS;
  return rc;
}

int ksmi_runner_mark_side(void* r_, int tag, int side_ix) {
  Runner* r = (Runner*)r_;
  if (!r) return ksmi_fail(KSMI_E_ARG, "runner_mark_side: null runner");
  return r->mark_side(tag, side_ix);
}

int ksmi_runner_wait_side(void* r_, int lane, int cur_lane, int tag) {
  Runner* r = (Runner*)r_;
  if (!r) return ksmi_fail(KSMI_E_ARG, "runner_wait_side: null runner");
  return r->wait_side(lane, cur_lane, tag);
}

int ksmi_runner_join(void* r_) {
  Runner* r = (Runner*)r_;
  if (!r) return ksmi_fail(KSMI_E_ARG, "runner_join: null runner");
  int rc = 0;
  if (r->dirty) {
    for (hipStream_t s : {r->lane1, r->side, r->side2})
      if (s && s != r->main && (rc = r->order(s, r->main))) return rc;
  }
  r->dirty = r->side_busy = false;
  for (auto& kv : r->tagged) r->tag_pool.push_back(kv.second);
  r->tagged.clear();
  r->cur = 0;
  return 0;
}

}  // extern "C"
