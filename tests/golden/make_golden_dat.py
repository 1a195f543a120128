"""Fixture of the packed-record input of sast_amd.events.EventQueue.push_dat: `python tests/golden/make_golden_dat.py` -> dat_events.npz.

The records are Prophesee's Event2D (8 bytes: u4 t, i4 x | y << 14 | p << 28), generated from `stream()`'s integer hash; the expected
columns are what the reference's own reader, load_td_data (utils/evaluation/prophesee/io/dat_events_tools.py:23-50), returns for a
.dat file that holds them.  The file's header is written by hand here: the reference's write_header names an undefined EV_STRINGS and
cannot run.  The records cover bits 29-31 set (the reader ignores them), t >= 2^31 (the time word is unsigned) and x, y up to 16383.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_events import _hash  # noqa: E402

OUT = os.path.join(HERE, "dat_events.npz")
N, H, W = 2048, 48, 80
T_START = (1 << 31) - 3000           # the clock passes 2^31 inside the recording


def records() -> np.ndarray:
    """-> int32 [N, 2].  Most events lie on the 48 x 80 sensor of the event tests; one in 16 anywhere in the format's 14-bit range"""
    far = _hash(91, N, 1) % np.uint64(16) == 0
    x = np.where(far, _hash(91, N, 2) % np.uint64(16384), _hash(91, N, 3) % np.uint64(W)).astype(np.int64)
    y = np.where(far, _hash(91, N, 4) % np.uint64(16384), _hash(91, N, 5) % np.uint64(H)).astype(np.int64)
    x[7], y[7], x[8], y[9] = 16383, 16383, 16383, 16383
    p = (_hash(91, N, 6) & np.uint64(1)).astype(np.int64)
    high = (_hash(91, N, 7) % np.uint64(8)).astype(np.int64)           # bits 29-31: 0 .. 7
    t = T_START + np.cumsum((_hash(91, N, 8) % np.uint64(4)).astype(np.int64))
    back = (_hash(91, N, 9) % np.uint64(16) == 0) & (np.arange(N) > 0)
    t[back] -= (_hash(91, N, 10)[back] % np.uint64(40)).astype(np.int64)
    w1 = x | (y << 14) | (p << 28) | (high << 29)
    return np.stack([t, w1], 1).astype(np.uint32).view(np.int32)


def load_reader():
    import _ref_import as RI
    path = os.path.join(RI.REF_ROOT, "utils", "evaluation", "prophesee", "io", "dat_events_tools.py")
    spec = importlib.util.spec_from_file_location("_ref_dat_events_tools", path)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod


def generate() -> dict:
    rec = records()
    reader = load_reader()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "fixture_td.dat")
        with open(path, "wb") as f:
            f.write(b"% Data file containing Event2D events.\n% Version 2\n% Date 2020-01-01 00:00:00\n% Height 16384\n% Width 16384\n")
            f.write(bytes([0, 8]))                                     # event type 0, 8 bytes per event
            f.write(rec.astype("<i4").tobytes())
        dat = reader.load_td_data(path)
    assert len(dat) == N
    return {"records": rec, "x": dat["x"].astype(np.int16), "y": dat["y"].astype(np.int16), "p": dat["p"].astype(np.int16),
            "t": dat["t"].astype(np.uint32)}


if __name__ == "__main__":
    data = generate()
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(data)} arrays")
