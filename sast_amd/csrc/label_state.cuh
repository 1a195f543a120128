// THE reader of the device state sast_labels_load leaves behind (include/sast_hip.h, SastLabelArgs): the label gather of k_labels.hip,
// the random-access sampler (k_sampler.hip) and the streaming sampler (k_stream.hip) all ask "what does row r hold at window w?" here.
// Every size is clamped when the row view is made and every index when it is formed, so nothing past a row's windows, frames or label
// rows is read, whatever the state holds: a count never exceeds the row's label rows, and [start, start + count) lies inside them.
//
// Plain C++ over the arguments alone (no thread index, no atomics, no HIP builtin): a host compiler builds this header as it stands,
// which is how tests/test_label_streams.py runs it over hostile states under the host sanitizers.
#pragma once
#include <stdint.h>
#include "../../include/sast_hip.h"

#ifdef __HIPCC__
#define SAST_HD __host__ __device__ __forceinline__
#else
#define SAST_HD inline
#endif

namespace sast {

SAST_HD int clampi(int v, int lo, int hi) {           // min(max(v, lo), hi): hi wins where lo > hi
  const int t = v < lo ? lo : v;
  return t > hi ? hi : t;
}

// the fields of the state every reader needs, and the sizes that keep its indices inside 32 bits
SAST_HD bool label_state_ok(const SastLabelArgs* a) {
  return a && a->ends_us && a->n_windows && a->n_frames && a->frame_2_window && a->window_2_frame && a->labels && a->frame_start &&
         a->frame_count && a->S >= 1 && a->S <= 65535 && a->capacity >= 1 && (long long)a->S * a->capacity <= INT32_MAX / 16 &&
         a->max_frames >= 1 && a->max_windows >= 1 && a->max_labels_per_frame >= 1 && (long long)a->S * a->max_frames <= INT32_MAX &&
         (long long)a->S * a->max_windows <= INT32_MAX;
}

struct LabelStep {         // one window of a row
  int labelled;            // 1: the window ends at a label frame (even one whose boxes all vanished)
  int count, start;        // its boxes: rows [start, start + count) of the row's label rows, count <= Mc
};

struct LabelRow {          // row r of the state, made once per (args, row) by label_row
  const int32_t* window_2_frame;
  const int32_t* frame_count;
  const int32_t* frame_start;
  const int64_t* ends_us;
  const int64_t* frame_2_window;
  const float* labels;
  int nw, nf;              // the row's windows and frames, inside [0, max_windows] / [0, max_frames]; a row without windows has no frames
  int Mc;                  // boxes one frame can hold: min(max_labels_per_frame, capacity)
  int max_frames, capacity;

  // w in [0, nw).  A frame id outside [0, max_frames) is no label frame.
  SAST_HD LabelStep step(long long w) const {
    LabelStep s = {0, 0, 0};
    const int f = window_2_frame[w];
    if (f >= 0 && f < max_frames) {
      s.labelled = 1;
      s.count = clampi(frame_count[f], 0, Mc);
      s.start = clampi(frame_start[f], 0, capacity - s.count);
    }
    return s;
  }
  SAST_HD const float* rows(const LabelStep& s) const { return labels + (int64_t)s.start * 7; }
  // out[M][7] <- the step's rows, zeros behind them: elements tid, tid + stride, ...
  SAST_HD void copy(const LabelStep& s, float* out, int M, int tid, int stride) const {
    const float* src = rows(s);
    for (int i = tid; i < M * 7; i += stride) out[i] = i < s.count * 7 ? src[i] : 0.f;
  }
};

SAST_HD LabelRow label_row(const SastLabelArgs& a, int r) {
  LabelRow v;
  v.window_2_frame = a.window_2_frame + (int64_t)r * a.max_windows;
  v.frame_count = a.frame_count + (int64_t)r * a.max_frames;
  v.frame_start = a.frame_start + (int64_t)r * a.max_frames;
  v.ends_us = a.ends_us + (int64_t)r * a.max_windows;
  v.frame_2_window = a.frame_2_window + (int64_t)r * a.max_frames;
  v.labels = a.labels + (int64_t)r * a.capacity * 7;
  v.nw = clampi(a.n_windows[r], 0, a.max_windows);
  v.nf = v.nw == 0 ? 0 : clampi(a.n_frames[r], 0, a.max_frames);
  v.Mc = (int)(a.max_labels_per_frame < a.capacity ? a.max_labels_per_frame : a.capacity);
  v.max_frames = a.max_frames;
  v.capacity = (int)a.capacity;
  return v;
}

}  // namespace sast
