"""What `LabelStreams.labels` gives for the (row, window) pairs of a pool's batch: the yardstick `RandomAccessPool.batch` and
`StreamingPool.next` are held to (tests/test_random_access.py, tests/test_streaming_pool.py)."""
import torch


def labels_of(ls, out, R):
    """LabelStreams.labels at (rows, window_idx) of a batch -> per batch row the four tensors, and which steps are real"""
    rows, widx = out.rows.tolist(), out.window_idx
    res = []
    for b, r in enumerate(rows):
        if r < 0:
            res.append(None)
            continue
        per_row = torch.zeros(widx.shape[0], R, dtype=torch.int64, device="cuda")
        per_row[:, r] = widx[:, b].clamp(min=0)
        labels, counts, ends, labelled = ls.labels(per_row)
        res.append((labels[:, r], counts[:, r], ends[:, r], labelled[:, r]))
    return res
