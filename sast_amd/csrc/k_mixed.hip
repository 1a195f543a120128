// The merged batch of `sampling: 'mixed'` (include/sast_hip.h, "mixed sampler"): Bs streamed rows and Br random-access samples in
// one batch of B = Bs + Br columns, stream columns first.
//
// The reference builds it on the CPU: set_mixed_sampling_mode_variables_for_train (modules/data/genx.py:116-129) splits the batch size,
// merge_mixed_batches (modules/utils/detection.py:133-161) concatenates the two loaders' batches along the batch axis, and training_step
// runs one forward and backward over the result, the random rows being reset every step (is_first_sample is true for them).  Here one
// launch writes both halves straight into the union tensors: workgroups [0, Bs) each walk a streamed row's L steps
// (stream_walk_row), the remaining Br * L workgroups each take one (step, random sample) (rnd_gather_step) -- the same two bodies
// sast_stream_next and sast_rnd_gather run, with the batch stride B and the random columns offset by Bs.  No workgroup reads what
// another one writes and nothing but the stream cursors is kept between calls, so the call replays inside a graph.
#include "common.cuh"
#include "kernels.h"
#include "label_state.cuh"
#include "sampler_rows.cuh"

namespace sast {
namespace {

__global__ __launch_bounds__(SAMPLER_THREADS) void mixed_next_kernel(SastLabelArgs a, SastStreamArgs qs, SastRndArgs qr, int Bs, int Br,
                                                                     const long long* items, StreamNextOut so, float* latest,
                                                                     int* latest_count) {
  const int blk = blockIdx.x, B = Bs + Br;
  if (blk < Bs) {                                             // uniform over the workgroup: the barrier inside is met by all of it
    stream_walk_row(a, qs, blk, B, blk, so);
    return;
  }
  const int i = blk - Bs, b = i % Br, k = i / Br, col = Bs + b;
  const RndGatherOut ro = {so.rows, so.step_rows, so.window_idx, so.ends_us, so.labels, so.counts, so.labelled, so.is_padded, latest, latest_count};
  rnd_gather_step(a, qr, items[b], k, B, col, b, ro);
  if (k == 0 && threadIdx.x == 0) {                           // a random sample is a first sample of its own and never runs out
    so.seq[col] = -1;
    so.sample[col] = -1;
    so.is_first[col] = 1;
    so.exhausted[col] = 0;
  }
}

}  // namespace
}  // namespace sast

extern "C" {

int sast_mixed_next(const SastLabelArgs* a, const SastStreamArgs* qs, const SastRndArgs* qr, int Bs, const int64_t* items, int Br, int32_t* rows,
                    int32_t* step_rows, int32_t* seq, int32_t* sample, uint8_t* is_first, uint8_t* exhausted, int64_t* window_idx,
                    int64_t* ends_us, float* labels, int32_t* counts, uint8_t* labelled, uint8_t* is_padded, float* latest,
                    int32_t* latest_count, sast_stream_t stream) {
  SAST_ENTRY();
  if (!sast::label_state_ok(a) || !sast::stream_args(qs) || !sast::stream_schedule_args(qs, Bs) || !sast::rnd_args(qr) || !items || Br < 1 ||
      !rows || !step_rows || !seq || !sample || !is_first || !exhausted || !window_idx || !ends_us || !labels || !counts || !labelled ||
      !is_padded || !latest || !latest_count)
    return SAST_EINVAL;
  if (qs->sequence_length != qr->sequence_length) return SAST_EINVAL;
  if (!sast::sampler_batch_fits((long long)Bs + Br, qs->sequence_length, a->max_labels_per_frame)) return SAST_EINVAL;
  const sast::StreamNextOut so = {rows, step_rows, seq, sample, is_first, exhausted, reinterpret_cast<long long*>(window_idx),
                                  reinterpret_cast<long long*>(ends_us), labels, counts, labelled, is_padded};
  const unsigned grid = (unsigned)Bs + (unsigned)Br * (unsigned)qs->sequence_length;
  SAST_LAUNCH(sast::mixed_next_kernel, dim3(grid), dim3(sast::SAMPLER_THREADS), 0, (hipStream_t)stream, *a, *qs, *qr, Bs, Br,
              reinterpret_cast<const long long*>(items), so, latest, latest_count);
  SAST_CHECK_LAUNCH();
  return SAST_OK;
}

}  // extern "C"
