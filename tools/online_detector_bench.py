"""Timing of online detection: `OnlineDetector.push` to the detections on the host (sast_amd/online.py), eager and as a replayed
graph, beside the hand-written loop of INTEGRATION.md section 3b completed by hand, on the same events, in the same process.

Gen4 sensor (720 x 1280, downsampled by 2), 50 ms windows, --windows windows of --events events per recording, chunks of a quarter
window, S in --streams; the detector is the benchmark's (embed_dim 64, PAFPN depth 0.67, 3 classes) with untrained weights, so the
number of detections says nothing (the records column: with the default initialisation no score reaches the threshold, and the
post-processing and the export run on empty rows).  Every recording runs on the same clock here, so that the hand loop, which cannot batch streams
whose windows fall due at different moments, has the same batches as the OnlineDetector.  Three sessions over the same chunks:
  hand      queue push, a host-side `while next_end < last_t:` over the due windows (one `frames` call, detector forward,
            `postprocess_padded`, `.cpu()` of the padded detections and their counts each), measured first
  eager     od.push(...) then od.drain()
  replayed  the chunk copied into the captured call's tensors (device to device), od.replay(), od.drain()
Wall-clock time of one chunk from the call to the results on the host, median (min .. max) over the session's chunks after the first
window, for all chunks and for those that complete a window.  An OnlineDetector push runs its W = 1 detector step whether a window is
due or not; the hand loop runs none for three chunks in four.  The chunks are already in device memory.

  python tools/online_detector_bench.py [--streams 1,8] [--windows 6] [--events 200000] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from event_streams_bench import H, W, WINDOW_US, synthetic  # noqa: E402

CHUNKS_PER_WINDOW, NUM_CLASSES, CONF, NMS, MAX_DET = 4, 3, 0.001, 0.45, 100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,8")
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--events", type=int, default=200000, help="events per recording and window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from sast_amd import functional as SF
    from sast_amd.config import backbone_config, modified_hw, to_attr
    from sast_amd.detection import YoloXDetector
    from sast_amd.events import EventQueue
    from sast_amd.online import OnlineDetector
    if not torch.cuda.is_available():
        raise SystemExit("tools/online_detector_bench.py needs a GPU: nothing is measured without one")
    dev = torch.device("cuda")
    props = torch.cuda.get_device_properties(0)
    T, E = a.windows, a.events
    chunk = E // CHUNKS_PER_WINDOW
    hw, part = modified_hw((H // 2, W // 2))
    torch.manual_seed(0)
    det = YoloXDetector(to_attr({"backbone": backbone_config(hw, part, embed_dim=64, AMP=2e-4, ls_init_value=1e-5),
                                 "fpn": {"name": "PAFPN", "depth": 0.67, "in_stages": [2, 3, 4], "depthwise": False, "act": "silu"},
                                 "head": {"name": "YoloX", "depthwise": False, "act": "silu", "num_classes": NUM_CLASSES}})).to(dev).eval()
    lines = [f"# tools/online_detector_bench.py on {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch "
             f"{torch.__version__}; Gen4 720 x 1280 downsampled by 2, 50 ms windows, {T} windows of {E} synthetic events per recording, chunks "
             f"of {chunk} events per row, windows_per_step 1, max_det {MAX_DET}; wall-clock ms per chunk from the call to the results on the "
             f"host, median (min .. max) over the chunks after the first window",
             "# hand: push + host-side while over due windows (frames, detector, postprocess_padded, .cpu());  eager: od.push + od.drain;  "
             "replayed: chunk copied into the captured tensors + od.replay + od.drain;  'due': the chunks that complete a window only",
             f"{'S':>3}  {'hand, all':<24}{'hand, due':<24}{'eager, all':<24}{'eager, due':<24}{'replayed, all':<24}{'replayed, due':<24}{'records hand/eager/replayed':>8}"]
    kw = dict(height=H, width=W, bins=10, count_cutoff=10, duration_us=WINDOW_US, downsample_by_2=True)
    for S in (int(v) for v in a.streams.split(",")):
        cols, ends = synthetic(S, T, E, seed=100 * S + T)
        start = ends[0:1].T - WINDOW_US                                    # one clock for all rows: window k ends at (k + 1) * 50 ms
        cols[3] = torch.clamp(cols[3] - start, min=0)
        n = T * E
        cuts = [(lo, min(lo + chunk, n)) for lo in range(0, n, chunk)]
        assert len(cuts) == T * CHUNKS_PER_WINDOW, "--events must be a multiple of 4"
        chunks = [[c[:, lo:hi].to(d).contiguous().to(dev) for c, d in zip(cols, (torch.int16,) * 3 + (torch.int32,))] for lo, hi in cuts]
        last_t = [int(np.maximum.accumulate(cols[3].numpy(), axis=1)[:, hi - 1].min()) for _lo, hi in cuts]   # the host's view of each chunk's end
        counts = torch.full((S,), chunk, dtype=torch.int64, device=dev)
        cap = 7 * E // 2

        def queue():
            return EventQueue(S, cap, window_capacity=2 * E, **kw)

        def hand():
            """section 3b's loop, completed: the FPN, the head, the post-processing and the way to the host"""
            q, end = queue(), torch.zeros(S, dtype=torch.int64, device=dev)
            next_end, states, times, n_rec = WINDOW_US, None, [], 0
            for i, cols_i in enumerate(chunks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                q.push(*cols_i, counts)
                n_due = 0
                while next_end < last_t[i]:
                    end.fill_(next_end)
                    frames = q.frames(end)
                    if states is None:
                        states = [(torch.zeros_like(h), torch.zeros_like(c)) for h, c in det(frames, None)[2]]
                    out, _losses, states, _p = det(frames, states)
                    d7, n7 = SF.postprocess_padded(out, NUM_CLASSES, CONF, NMS)
                    d7, n7 = d7.cpu(), n7.cpu()
                    n_rec += int(n7.clamp(max=MAX_DET).sum())
                    next_end += WINDOW_US
                    n_due += 1
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0, n_due))
            return times, n_rec

        def online(replayed):
            od = OnlineDetector(det, queue(), windows_per_step=1, max_det=MAX_DET, conf_thre=CONF, nms_thre=NMS)
            static = [torch.zeros_like(c) for c in chunks[0]]
            times, n_rec = [], 0
            for i, cols_i in enumerate(chunks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if replayed and i > 0:
                    for dst, src in zip(static, cols_i):
                        dst.copy_(src)
                    od.replay()
                elif replayed:
                    for dst, src in zip(static, cols_i):
                        dst.copy_(src)
                    od.push(*static, counts)
                else:
                    od.push(*cols_i, counts)
                res = od.drain()
                times.append((time.perf_counter() - t0, len(res)))
                n_rec += sum(len(r) for _s, r in res)
                if replayed and i == 0:
                    od.capture()
            assert od.errors()[:4] == (0, 0, 0, 0), od.errors()
            return times, n_rec

        with torch.no_grad():
            hand()                                                      # warm-up: code objects, workspaces, the allocator's blocks
            res = [hand(), online(False), online(True)]
        # the last window is never due here (no event later than its end arrives): every form gives T - 1 windows per row.  A row whose
        # chunk ends just before a window end gives that window one push later than its neighbours: the hand loop waits for the slowest row

        def cell(times, due_only):
            v = [1e3 * t for i, (t, k) in enumerate(times) if i >= CHUNKS_PER_WINDOW + 1 and (k > 0 or not due_only)]
            return f"{statistics.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})" if v else "-"

        lines.append(f"{S:>3}  " + "".join(f"{cell(r[0], d):<24}" for r in res for d in (False, True)) + f"{'/'.join(str(r[1]) for r in res):>8}")
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
