"""Scene-adaptive selection restated in plain torch, in any float dtype: what `sast_select`, `sast_select_pair` and `sast_select_packs`
(csrc/k_select.hip) must produce, field by field of `SastSel` (include/sast_hip.h).  CPU only; independent of oracle/sast_oracle.py
(tests/test_selection_reference.py compares the two).

From the per-token scores tok [B, L] (L = H * W, image order), the partition (ph, pw), the mode (0: windows are contiguous ph x pw tiles,
1: a grid group takes one token from each of the ph x pw coarse cells) and bounce:
  window score   mean of the T = ph * pw token scores of a group (the L1 norm / T of the reference; scores are >= 0)
  window keep    softmax over the N groups of a sample >= (1 / N) / (1 + bounce)
  token keep     in a kept window, softmax over its T tokens >= (1 / T) / (1 + bounce)
Both thresholds are evaluated in Python doubles and rounded ONCE to the dtype the softmax is held in -- to float32 for the kernels and the
float32 restatement, which is the tensor-against-Python-scalar compare of the reference.  (In float64 the threshold stays the double: a
uniform map, whose softmax values are exactly fl(1 / N), then sits exactly on its threshold at bounce 0 in either precision.)

Compact rows: kept tokens in flat group order w = b * N + n, ascending slot inside a group.  Attention packs: see `packs`.
"""
import torch

SEG_SHIFT = 16


def group_token_ids(H, W, ph, pw, mode):
    """[N, T] token index l = y * W + x of slot t of group n"""
    gh, gw = H // ph, W // pw
    idx = torch.arange(H * W).view(H, W)
    if mode == 0:
        g = idx.view(gh, ph, gw, pw).permute(0, 2, 1, 3)
    else:
        g = idx.view(ph, gh, pw, gw).permute(1, 3, 0, 2)
    return g.reshape(gh * gw, ph * pw)


def thresholds(N, T, bounce, dtype):
    return (torch.tensor((1.0 / N) / (1.0 + bounce), dtype=dtype), torch.tensor((1.0 / T) / (1.0 + bounce), dtype=dtype))


def softmax(x):
    e = torch.exp(x - x.max(-1, keepdim=True)[0])
    return e / e.sum(-1, keepdim=True)


def probabilities(tok, B, H, W, ph, pw, mode, dtype):
    """(nw [B, N], nt [B * N, T]): the two softmax maps every decision is read from"""
    gid = group_token_ids(H, W, ph, pw, mode)
    g = tok.to(dtype).view(B, H * W)[:, gid]                   # [B, N, T]
    nw = softmax(g.abs().sum(-1) / (ph * pw))
    nt = softmax(g.abs().reshape(B * gid.shape[0], ph * pw))
    return nw, nt


def pack_limit(T, knob=32):
    """rows an attention pack may hold: the SAST_ATTN_PACKS knob (default 32), capped by what the kernel instantiated for T holds"""
    cap = 64 if T <= 64 else (96 if T <= 96 else 128)
    return min(int(knob), cap)


def packs(K, limit):
    """(pack_rows [W], lo [W]) from the kept tokens per group.  The flat group order is cut into aligned blocks of 16 groups (they run
    across samples when N % 16 != 0; groups past W count as 0).  The pack of a group is the largest of the nested aligned sub-blocks of
    1, 2, 4, 8, 16 groups around it whose kept rows sum to at most `limit`: one group always fits, the first size that does not fit ends
    the search.  pack_rows[w]: rows of the pack if w is its first group, else 0.  lo[w]: rows of the pack in front of group w."""
    K = [int(k) for k in K]
    W = len(K)
    pack_rows, lo = [0] * W, [0] * W
    for b0 in range(0, W, 16):
        kk = [K[b0 + j] if b0 + j < W else 0 for j in range(16)]
        for i in range(min(16, W - b0)):
            lead, rows, before = i, kk[i], 0
            for sz in (2, 4, 8, 16):
                s0 = i - i % sz
                tot = sum(kk[s0:s0 + sz])
                if tot > limit:
                    break
                lead, rows, before = s0, tot, sum(kk[s0:i])
            lo[b0 + i] = before
            if lead == i:
                pack_rows[b0 + i] = rows
    return pack_rows, lo


def select(tok, B, H, W, ph, pw, mode, bounce, limit, dtype=torch.float64):
    """every field of SastSel as a CPU tensor (int32 like the device buffers; `bits` [B * N, T] bool for the mask words), plus the
    reference-style lists index_window / asy_index / K_list and `total`"""
    L, T = H * W, ph * pw
    gid = group_token_ids(H, W, ph, pw, mode)
    N = gid.shape[0]
    nw, nt = probabilities(tok, B, H, W, ph, pw, mode, dtype)
    thr_w, thr_t = thresholds(N, T, bounce, dtype)
    keep = (nw >= thr_w).reshape(B * N)
    bits = (nt >= thr_t) & keep[:, None]
    K = bits.sum(1)
    row_off = torch.cumsum(K, 0) - K
    total, M = int(K.sum()), int(keep.sum())
    win_rank = torch.where(keep, torch.cumsum(keep.long(), 0) - 1, torch.full_like(K, -1))
    image_tok = (torch.arange(B).view(B, 1, 1) * L + gid.view(1, N, T)).reshape(B * N, T)       # b * L + l of (group, slot)
    row_tok = image_tok[bits]                                   # row-major over (group, slot): group order, ascending slot
    tok_slot = torch.full((B * L,), -1, dtype=torch.long)
    tok_slot[row_tok] = torch.arange(total)
    pack_rows, lo = packs(K.tolist(), limit)
    lo = torch.tensor(lo, dtype=torch.long)
    row_group = torch.repeat_interleave(torch.arange(B * N), K)
    row_seg = lo[row_group] | ((lo + K)[row_group] << SEG_SHIFT)
    i32 = lambda t: t.to(torch.int32)      # noqa: E731
    return {"win_keep": i32(keep), "bits": bits, "K": i32(K), "row_off": i32(row_off), "win_rank": i32(win_rank),
            "counts": torch.tensor([total, M, total // B, 0], dtype=torch.int32), "tok_slot": i32(tok_slot), "row_tok": i32(row_tok),
            "pack_rows": torch.tensor(pack_rows, dtype=torch.int32), "row_seg": i32(row_seg), "total": total,
            "index_window": torch.nonzero(keep).view(-1), "asy_index": torch.nonzero(bits[keep].reshape(-1)).view(-1), "K_list": K[keep]}


FIELDS = ("win_keep", "bits", "K", "row_off", "win_rank", "counts", "tok_slot", "row_tok", "pack_rows", "row_seg")
LISTS = ("index_window", "asy_index", "K_list")


def margins(tok, B, H, W, ph, pw, mode, bounce):
    """relative distance of every decision of the float64 evaluation to its threshold: (window [B, N], token [B * N, T]).  A decision of
    an exactly uniform row (a constant map, an empty frame) counts as infinitely far: every value of such a row is fl(1 / n) in every
    precision and summation order (exp(0) = 1, a sum of n ones, one correctly rounded division), at or above the threshold for any
    bounce >= 0, so no evaluation can decide it differently."""
    nw, nt = probabilities(tok, B, H, W, ph, pw, mode, torch.float64)
    thr_w, thr_t = thresholds(nw.shape[1], nt.shape[1], bounce, torch.float64)
    out = []
    for p, thr in ((nw, thr_w), (nt, thr_t)):
        d = (p - thr).abs() / thr
        uniform = (p == p[..., :1]).all(-1, keepdim=True) & (p >= thr)
        out.append(torch.where(uniform.expand_as(d), torch.full_like(d, float("inf")), d))
    return out
