"""Timing of the event noise filters (`sast_amd.events.EventFilter`, csrc/k_evfilter.hip), all in this one process:

  filter    one filter call per mode ("activity" radius 1, "contrast"; threshold 10 ms) at 1280 x 720, S in --streams, chunks of
            --events events per row, beside the `Evt3Decoder` call that gives such a chunk from its EVT 3.0 words and the unfiltered
            `EventQueue.push` of it.  Synthetic chunks: pixels and polarities uniform, times sorted, 4 events per microsecond and row
            (no real sensor has been measured), already in device memory.  Every figure is the time of one call between two device
            events, the call captured in a graph and replayed (the GPU's time, not the host's issue rate).  A filter call is timed on
            the state the chunk in front left: the graph first copies that surface and carry back, and the median time of a graph
            of those copies alone is subtracted.  "sort share": the device time of the radix sort's kernels over the device time of
            all kernels of one eager call (the copies left out), from torch.profiler.
  push      one captured `OnlineDetector` push (windows_per_step 2) with and without a filter on its queue, on the detector and the
            synthetic Gen4 recordings of tools/online_detector_bench.py, two passes each, interleaved.

Medians after warm-up, (min .. max) behind them.

  python tools/event_filter_bench.py [--reps 10] [--streams 1,8] [--events 100000,1000000] [--out FILE] [--commit TEXT] [--no-push] [--no-filter]
"""
from __future__ import annotations

import argparse
import gc
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

H, W, THRESHOLD_US, RATE = 720, 1280, 10_000, 4


def med(v):
    return f"{statistics.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def chunk(S, n, seed):
    """one chunk of n events per row, on the device: x, y, p int16, t int64 sorted, counts"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randint(0, W, (S, n), generator=g, device="cuda").to(torch.int16)
    y = torch.randint(0, H, (S, n), generator=g, device="cuda").to(torch.int16)
    p = torch.randint(0, 2, (S, n), generator=g, device="cuda").to(torch.int16)
    t = 1000 + torch.sort(torch.randint(0, max(n // RATE, 1), (S, n), generator=g, device="cuda"), dim=1).values
    return [x, y, p, t], torch.full((S,), n, dtype=torch.int64, device="cuda")


def replay_ms(fn, reps):
    """ms per call of fn, captured once and replayed"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    out = []
    for _ in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out[2:]


def sort_share(fn):
    """(the sort's device time, all kernels' device time) of one eager call, us; None where the profiler gives no kernel times"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0)) for e in prof.key_averages()]
        rows = [(k, t) for k, t in rows if t > 0 and not any(w in k.lower() for w in ("memcpy", "memset", "copy", "elementwise"))]
        own = sum(t for k, t in rows if "evfilter_" in k)
        total = sum(t for _k, t in rows)
        return (total - own, total) if own > 0 else None
    except Exception as e:                                           # noqa: BLE001  (a measurement aid: say why it is missing)
        print(f"  (no sort share: {type(e).__name__}: {e})", flush=True)
        return None


def filter_section(streams, sizes, reps, lines):
    from sast_amd.events import EventFilter, EventQueue, Evt3Decoder, Evt3Encoder
    for S in streams:
        for n in sizes:
            prev, counts = chunk(S, n, seed=S * 1000 + n % 997)
            cols, _n = chunk(S, n, seed=S * 1000 + n % 997 + 1)
            cols[3] += max(n // RATE, 1)                              # the chunk that follows `prev` in time
            words, n_words = (v.clone() for v in Evt3Encoder(S)(*cols, counts))
            words = words[:, :int(n_words.max())].contiguous()
            dec = Evt3Decoder(S, max_events=n)
            q = EventQueue(S, 2 * n, H, W, duration_us=50_000, downsample_by_2=True)
            rst = torch.ones(S, dtype=torch.uint8, device="cuda")     # every replay starts the rows over: the same work each time
            t_dec = replay_ms(lambda: dec(words, n_words, rst), reps)
            t_push = replay_ms(lambda: q.push(*cols, counts, rst), reps)
            lines.append(f"filter, S {S}, {n} events per row ({float(n_words.float().mean()) / n:.2f} EVT 3.0 words per event), ms per call")
            lines.append(f"  Evt3Decoder             {med(t_dec)}")
            lines.append(f"  EventQueue.push         {med(t_push)}")
            base = statistics.median(t_dec) + statistics.median(t_push)
            del dec, q
            for mode in ("activity", "contrast"):
                f = EventFilter(S, H, W, mode=mode, threshold_us=THRESHOLD_US, radius=1)
                f(*prev, counts)                                      # a surface with history: the chunk in front of the timed one
                steady = [v.clone() for v in (f.surface, f.t_last)]

                def restore():
                    f.surface.copy_(steady[0]), f.t_last.copy_(steady[1])

                def call():
                    restore()
                    return f(*cols, counts)

                t_restore = statistics.median(replay_ms(restore, reps))
                t_f = [max(v - t_restore, 0.0) for v in replay_ms(call, reps)]
                f.seen.zero_(), f.kept.zero_()
                call()
                kept = float(f.kept.sum()) / float(f.seen.sum())
                share = sort_share(call)
                m = statistics.median(t_f)
                lines.append(f"  EventFilter {mode:9s}   {med(t_f)}   kept {kept:.3f}   {m / base:.2f} x decode + push   "
                             + (f"sort share {share[0] / share[1]:.2f} ({share[0] / 1e3:.3f} of {share[1] / 1e3:.3f} ms of kernels)"
                                if share else "sort share not measured"))
                del f
            torch.cuda.empty_cache()
            print("\n".join(lines[-5:]), flush=True)


def push_section(S, lines):
    import online_detector_bench as B
    from sast_amd.config import backbone_config, modified_hw, to_attr
    from sast_amd.detection import YoloXDetector
    from sast_amd.events import EventFilter, EventQueue
    from sast_amd.online import OnlineDetector
    dev, T, E, Wn, max_det = torch.device("cuda"), 8, 200000, 2, 100
    hw, part = modified_hw((B.H // 2, B.W // 2))
    torch.manual_seed(0)
    det = YoloXDetector(to_attr({"backbone": backbone_config(hw, part, embed_dim=64, AMP=2e-4, ls_init_value=1e-5),
                                 "fpn": {"name": "PAFPN", "depth": 0.67, "in_stages": [2, 3, 4], "depthwise": False, "act": "silu"},
                                 "head": {"name": "YoloX", "depthwise": False, "act": "silu", "num_classes": B.NUM_CLASSES}})).to(dev).eval()
    cols, ends = B.synthetic(S, T, E, seed=100 * S + T)
    cols[3] = torch.clamp(cols[3] - (ends[0:1].T - B.WINDOW_US), min=0)
    size = 2 * E                                                      # two windows per chunk: both steps of a push are due
    chunks = [[c[:, lo:lo + size].to(d).contiguous().to(dev) for c, d in zip(cols, (torch.int16,) * 3 + (torch.int32,))]
              for lo in range(0, T * E, size)]
    counts = torch.full((S,), size, dtype=torch.int64, device=dev)
    kw = dict(height=B.H, width=B.W, bins=10, count_cutoff=10, duration_us=B.WINDOW_US, downsample_by_2=True)
    rows = []
    for filtered in (False, True, False, True):
        f = EventFilter(S, B.H, B.W, mode="activity", threshold_us=THRESHOLD_US) if filtered else None
        od = OnlineDetector(det, EventQueue(S, 4 * size, window_capacity=2 * E, filter=f, **kw), windows_per_step=Wn, max_det=max_det,
                            conf_thre=0.3, nms_thre=0.45)
        static = [torch.zeros_like(c) for c in chunks[0]]
        wall, graph = [], []
        with torch.no_grad():
            for _rep in range(3):                                     # the recording again and again: reset at its first chunk
                for i, cols_i in enumerate(chunks):
                    reset = torch.full((S,), int(i == 0), dtype=torch.uint8, device=dev)
                    for dst, src in zip(static, cols_i):
                        dst.copy_(src)
                    if od._graph is None:
                        flags = reset.clone()
                        od.push(*static, counts, flags)
                        od.drain()
                        od.capture()
                        continue
                    flags.copy_(reset)
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    a.record()
                    od._graph.replay()
                    b.record()
                    od._copy_out()
                    od.drain()
                    wall.append(1e3 * (time.perf_counter() - t0))
                    graph.append(a.elapsed_time(b))
        kept = float(f.kept.sum()) / max(float(f.seen.sum()), 1.0) if filtered else 1.0
        rows.append((filtered, wall[2:], graph[2:], kept))
        # the detector object and its last push refer to each other: without this its graph would be destroyed by the cyclic collector at
        # a moment of its choosing, and destroying a graph while the next pass captures its own is refused by the runtime
        od._last = od._graph = None
        del od, f
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    lines.append(f"push, S {S}, windows_per_step {Wn}: one captured OnlineDetector push per chunk of two 50 ms windows (Gen4 / 2, {E} events "
                 f"per window and row), ms; two passes each, interleaved")
    for filtered, wall, graph, kept in rows:
        lines.append(f"  {'with filter   ' if filtered else 'without filter'}  graph alone {med(graph)}   replay to host {med(wall)}   kept {kept:.3f}")
    print("\n".join(lines[-5:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--streams", default="1,8")
    ap.add_argument("--events", default="100000,1000000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--no-push", action="store_true")
    ap.add_argument("--no-filter", action="store_true", help="the push section alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/event_filter_bench.py needs a GPU: nothing is measured without one")
    props = torch.cuda.get_device_properties(0)
    streams, sizes = [int(v) for v in a.streams.split(",")], [int(v) for v in a.events.split(",")]
    # the options that shape the measurement; where the table is written is not one of them
    lines = [f"# python tools/event_filter_bench.py --reps {a.reps} --streams {a.streams} --events {a.events}{' --no-push' if a.no_push else ''}{' --no-filter' if a.no_filter else ''}",
             f"# commit {a.commit}; {props.name} ({getattr(props, 'gcnArchName', '?')}, {props.multi_processor_count} CUs), torch {torch.__version__}; "
             f"medians (min .. max) after warm-up"]
    if not a.no_filter:
        filter_section(streams, sizes, a.reps, lines)
    if not a.no_push:
        push_section(max(streams), lines)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
