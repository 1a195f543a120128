"""Plain torch expressions of the token-path operators of `sast_amd.functional` (the transformer side of the backbone): STP scoring,
mask token, position-embedding add, the MS-WSA layer and the ConvLSTM.  CPU only; everything runs in the dtype of its inputs, so the same
expression is the float64 reference of tests/test_token_operators.py and, evaluated in float32, the yardstick of
tests/golden/make_operator_bounds.py.

MS-WSA and ConvLSTM are the oracle's functions (oracle/sast_oracle.py: ms_wsa, conv_lstm) behind a parameter-name mapping.  Scoring has no
stand-alone function there -- it is inline in `sast_block` (oracle/sast_oracle.py:339-354) -- and is written out here; so are the two
one-line operators.  tests/test_token_reference.py pins all three restatements against the oracle lines they restate.
"""
import torch
import torch.nn.functional as F

from oracle import sast_oracle as O


# ------------------------------------------------------------------------------------------------ STP scoring
def score_preact(xp, ws_w, ws_b):
    """pre-activation of the scoring linear (the argument of the ReLU whose gate the backward kernel evaluates as s > 0)"""
    return F.linear(xp, ws_w, ws_b)


def score_stp(xp, r, ws_w, ws_b, wc, amp):
    """oracle/sast_oracle.py:343-354 on rows that already carry the position embedding.  xp (B, L, C), r (B, 20), wc (C, 20)
    -> (xw (B, L, C), tok (B, L)): xw = sigmoid(scale) sigmoid(relu(z)) xp, tok = sum_c amp / scale * relu(z) with inf -> 0."""
    scale = F.linear(r + 1e-6, torch.exp(wc))[:, None, :]
    s = F.relu(score_preact(xp, ws_w, ws_b))
    xw = (scale.sigmoid() * s.sigmoid()) * xp
    inv = amp / scale
    inv = inv.masked_fill(inv == torch.inf, 0)
    return xw, (inv * s).sum(-1)


# ------------------------------------------------------------------------------------------------ mask token, position embedding
def add_pos_embedding(x, table):
    """oracle/sast_oracle.py:339: x (B, H, W, C) + table (1, H, W, C) repeated over the batch"""
    return x + table.reshape(1, *x.shape[1:])


def mask_token(x, mask, token, table=None):
    """oracle/sast_oracle.py:428-430 on rows that already carry the position embedding (the device order): a masked row becomes
    mask_token (+ its row of the table).  x (B, H, W, C), mask (B, H, W) bool, token (1, 1, 1, C), table (1, H, W, C) or None."""
    t = token.reshape(1, 1, 1, -1)
    if table is not None:
        t = t + table.reshape(1, *x.shape[1:])
    return torch.where(mask[..., None], t.expand_as(x), x)


# ------------------------------------------------------------------------------------------------ MS-WSA
MSWSA_NAMES = {"ln1_w": "norm1.weight", "ln1_b": "norm1.bias", "ln2_w": "norm2.weight", "ln2_b": "norm2.bias", "qkv_w": "qkv.weight",
               "qkv_b": "qkv.bias", "proj_w": "proj.weight", "proj_b": "proj.bias", "ls1": "ls1.gamma", "fc1_w": "mlp.net.0.proj.weight",
               "fc1_b": "mlp.net.0.proj.bias", "fc2_w": "mlp.net.2.weight", "fc2_b": "mlp.net.2.bias", "ls2": "ls2.gamma",
               "act_w": "mlp.net.0.act_layer.weight"}


def index_lists(kept, T):
    """reference-style lists of a selection given as {window id: sorted kept slots}: [index_window, index_token, padding_index,
    asy_index, K] (oracle/sast_oracle.py:167-177; the top-k fillers are the window's first unkept slots)"""
    wins = sorted(kept)
    Ks = [len(kept[w]) for w in wins]
    kmax = max(Ks) if Ks else 0
    rows, asy = [], []
    for m, w in enumerate(wins):
        kt = torch.as_tensor(kept[w], dtype=torch.long)
        rest = torch.as_tensor([t for t in range(T) if t not in set(kept[w])], dtype=torch.long)
        rows.append(m * T + torch.cat([kt, rest])[:kmax])
        asy.append(m * T + kt)
    cat = lambda l: torch.cat(l) if l else torch.zeros(0, dtype=torch.long)     # noqa: E731
    index_token, asy = cat(rows), cat(asy)
    padding = index_token[torch.isin(index_token, asy, invert=True)]
    return [torch.as_tensor(wins, dtype=torch.long), index_token, padding, asy, torch.as_tensor(Ks, dtype=torch.long)]


def mswsa(x, lists, B, p, dim_head, eps=1e-5, cb=False, act="gelu", drop=None):
    """oracle.ms_wsa on x (B * N, T, C) in partitioned layout.  p: device names (MSWSA_NAMES keys); ls1 / ls2 None = LayerScale
    disabled (the oracle multiplies by a vector of ones, which is exact).  drop: None or (d1, d2, mlp_mask) for the KEPT rows, in the
    oracle's order of use (attention branch, MLP hidden, MLP branch); None entries are off."""
    C = x.shape[-1]
    po = {MSWSA_NAMES[k]: v for k, v in p.items() if v is not None}
    for k in ("ls1.gamma", "ls2.gamma"):
        po.setdefault(k, torch.ones(C, dtype=x.dtype))
    d1, d2, dm = drop if drop is not None else (None, None, None)
    masks = [m.to(x.dtype) for m in (d1, dm, d2) if m is not None]
    cfg = O.AttnCfg(partition_size=(x.shape[1], 1), dim_head=dim_head, norm_eps=eps, enable_cb=cb, mlp_activation=act,
                    drop_path=0.5 if d1 is not None else 0.0, drop_mlp=0.5 if dm is not None else 0.0, training=True,
                    drop_masks=masks if masks else None)
    return O.ms_wsa(x, lists, B, po, "", cfg)


# ------------------------------------------------------------------------------------------------ ConvLSTM
def nchw(x):
    return x.permute(0, 3, 1, 2)


def nhwc(x):
    return x.permute(0, 2, 3, 1)


def conv_lstm(x, h0, c0, w, b, drop=None):
    """oracle.conv_lstm (NCHW) on NHWC tensors: x, h0, c0, drop (B, H, W, C) (h0 / c0 None = zero state), w (4C, 2C, 1, 1), b (4C,)
    -> (h1, c1) NHWC"""
    z = torch.zeros_like(x)
    hc = (nchw(h0 if h0 is not None else z), nchw(c0 if c0 is not None else z))
    h1, c1 = O.conv_lstm(nchw(x), hc, {"conv1x1.weight": w, "conv1x1.bias": b}, "", drop_mask=nchw(drop) if drop is not None else None)
    return nhwc(h1), nhwc(c1)
