"""The argument rules and per-row state helpers of the device-resident data front end (`events.py`, `sampling.py`, `labels.py`,
`online.py`; `augment.py` and `evaluation.py` for the two sentences they share), each held once: one function, one sentence, prefixed
with the module that raises it.  The rules look at shape, dtype and layout only, so a caller applies them to CPU tensors too, before
`_need_gpu`'s "no CPU fallback" error.  Nothing here launches a kernel, and only `counters` (the `errors()` methods) synchronises.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib as L
from .functional import _need_gpu

_EV_DT = {torch.int64: L.DT_I64, torch.int32: L.DT_I32, torch.int16: L.DT_I16}


def _dt(dtype: torch.dtype) -> str:
    return str(dtype).replace("torch.", "")


def _fits(have, want, low: int) -> bool:
    if len(have) != len(want):
        return False
    for n, d in zip(have, want):
        if n != d and (n < low if isinstance(d, str) else n != d[1] if isinstance(d, tuple) else True):
            return False
    return True


def tensor_arg(t, name: str, module: str, dtypes, shape, what: Optional[str] = None, empty_ok: bool = False, device=None,
               dtype_error=ValueError) -> None:
    """`t` is a contiguous tensor of one of `dtypes` (None: any) and of `shape`, on `device` where one is given.

    shape: a tuple of dimensions, or a list of such tuples where several ranks are taken.  A dimension is an int (that size), a
    string (a free size, printed as it is: >= 1, >= 0 with empty_ok) or a (string, int) pair (that size, printed as `string=int`).
    what: words put behind the shape ("on the queue's device").  A wrong dtype raises `dtype_error`, everything else ValueError.
    This runs in front of every launch: the passing path is a few comparisons."""
    shapes = shape if isinstance(shape, list) else (shape,)
    tensor, fits = isinstance(t, torch.Tensor), False
    if tensor:
        have, low = t.shape, 0 if empty_ok else 1
        for s in shapes:
            if have == s or _fits(have, s, low):
                fits = True
                break
    if fits and t.is_contiguous() and (dtypes is None or t.dtype in dtypes) and (device is None or t.device == device):
        return
    bad = ValueError
    if not tensor:
        got = f"a {type(t).__name__}"
    elif not fits or (dtypes is not None and t.dtype not in dtypes):
        got, bad = f"{_dt(t.dtype)} {list(t.shape)}", dtype_error if fits else ValueError
    elif not t.is_contiguous():
        got = f"strides {list(t.stride())}"
    else:
        got = f"a tensor on {t.device}"
    free = [] if empty_ok else list(dict.fromkeys(d for s in shapes for d in s if isinstance(d, str)))
    dims = " or ".join("[" + ", ".join("=".join(map(str, d)) if isinstance(d, tuple) else str(d) for d in s) + "]" for s in shapes)
    raise bad(f"sast_amd.{module}: {name} must be a contiguous {' or '.join(_dt(d) for d in dtypes or ())}{' ' if dtypes else ''}tensor "
              f"of shape {dims}{''.join(f', {d} >= 1' for d in free)}{' ' + what if what else ''}, got {got}")


def stream_count(num_streams, module: str) -> int:
    """rows are grid.y of the per-row kernels"""
    if int(num_streams) < 1 or int(num_streams) > 65535:
        raise ValueError(f"sast_amd.{module}: num_streams must be in 1 .. 65535")
    return int(num_streams)


def dtype_code(t: torch.Tensor, name: str, module: str, allowed=(torch.int64, torch.int32, torch.int16)) -> int:
    """the library's code of an event column's dtype"""
    if t.dtype not in allowed:
        raise TypeError(f"sast_amd.{module}: {name} must be one of {[str(d) for d in allowed]}, got {t.dtype}")
    return _EV_DT[t.dtype]


def event_columns(x, y, p, t, rows: int, module: str, rows_name: str = "num_streams", cap_name: str = "capacity"):
    """x, y, p, t are contiguous [rows, capacity] tensors of one shape (capacity 0: an empty chunk) -> their four dtype codes"""
    spec = ((rows_name, rows), cap_name)
    tensor_arg(x, "x", module, None, spec, empty_ok=True)
    same = True
    for c, name in ((y, "y"), (p, "p"), (t, "t")):
        if not (isinstance(c, torch.Tensor) and c.shape == x.shape and c.is_contiguous()):       # else: it keeps the rule x has passed
            tensor_arg(c, name, module, None, spec, empty_ok=True)
            same = False
    if not same:
        raise ValueError(f"sast_amd.{module}: x, y, p and t must have the same shape")
    codes = [_EV_DT.get(c.dtype) for c in (x, y, p, t)]
    if None in codes or codes[3] == L.DT_I16:                 # name the column: x, y, p int64 / int32 / int16, t int64 / int32
        dtype_code(x, "x", module), dtype_code(y, "y", module), dtype_code(p, "p", module)
        dtype_code(t, "t", module, (torch.int64, torch.int32))
    return codes


def flags(t, name: str, rows: int, module: str) -> None:
    """an optional per-row flag tensor (`reset`, `final`): uint8 / bool [rows]"""
    if t is not None:
        tensor_arg(t, name, module, (torch.uint8, torch.bool), (rows,))


def counts_reset(counts, reset, rows: int, module: str) -> None:
    """per-row event (word, record) counts int64 [rows], and the optional flags of the rows that start a new recording"""
    tensor_arg(counts, "counts", module, (torch.int64,), (rows,))
    flags(reset, "reset", rows, module)


def window_ends(ends_us, S: int, module: str, name: str = "ends_us") -> int:
    """window ends (or indices) for S rows, int64 [S] or [T, S] -> T"""
    tensor_arg(ends_us, name, module, (torch.int64,), [(S,), ("T", S)])
    return ends_us.shape[0] if ends_us.dim() == 2 else 1


def same_device(module: str, names: str, *tensors) -> None:
    """the tensors given (None: an optional one that was left out) are on one device; `names` is how the sentence lists them"""
    if len({t.device for t in tensors if t is not None}) > 1:
        raise ValueError(f"sast_amd.{module}: {names} must be on the same device")


def lives_on(owner: str, dev, what: str, got, module: str) -> None:
    """state that was allocated on `dev` is not moved: the call's tensors must be there too"""
    if got != dev:
        raise ValueError(f"sast_amd.{module}: {owner} lives on {dev}, {what} on {got}")


def not_capturing(module: str, what: str = "one un-captured warm-up call is needed before graph capture") -> None:
    """buffers are allocated outside graph capture only: the first call with new sizes must be an ordinary one"""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"sast_amd.{module}: {what}")


def frames_out(out, shape, dtype, dev, module: str, name: str, owner: str) -> torch.Tensor:
    """the tensor a frames call writes: a new one, or the caller's checked against what a new one would be"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    tensor_arg(out, name, module, (dtype,), tuple(shape), f"on {owner} device", device=dev)
    return out


def outputs(cls, want, out, dev, module: str, what: str, owner: str):
    """the tensors a gather call writes, as a `cls` (a NamedTuple class): allocated as `want` says ((shape, dtype) per field), or the
    caller's `out` checked against it"""
    if out is None:
        return cls(*(torch.empty(sh, dtype=dt, device=dev) for sh, dt in want))
    out = tuple(out)
    if len(out) != len(want):
        raise ValueError(f"sast_amd.{module}: out must be the {what}")
    _need_gpu(*out)
    for t, (sh, dt), name in zip(out, want, cls._fields):
        tensor_arg(t, f"out's {name}", module, (dt,), sh, f"on {owner} device", device=dev)
    return cls(*out)


def reset_rows(state: Sequence[Optional[torch.Tensor]], counters: Optional[torch.Tensor], streams, num_streams: int, module: str) -> None:
    """new recordings, from the host: rows `streams` of every per-row tensor of `state` back to zero; with streams=None every row, and
    the `counters` as well.  Nothing to do while the state is not allocated."""
    if state[0] is None:
        return
    if streams is None:
        for v in state:
            v.zero_()
        counters.zero_()
        return
    idx = [int(s) for s in streams]
    if any(s < 0 or s >= num_streams for s in idx):
        raise ValueError(f"sast_amd.{module}: streams must be in 0 .. {num_streams - 1}")
    if idx:
        sel = torch.tensor(idx, dtype=torch.int64, device=state[0].device)
        for v in state:
            v[sel] = 0


def counters(err: Optional[torch.Tensor], n: int) -> Tuple[int, ...]:
    """what an `errors()` method returns: the n device counters (synchronises), zeros while they are not allocated"""
    return (0,) * n if err is None else tuple(int(v) for v in err.tolist())
