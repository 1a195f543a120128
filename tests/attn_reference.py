"""Plain torch expression of the variable-length window attention of sast_amd/csrc/k_attn_mfma.hip (attn_fwd_mfma_launch /
attn_bwd_mfma_launch) on compact rows.  CPU only; everything runs in the dtype of its inputs, so the same expression is the float64
reference of tests/test_attn_operators.py and, evaluated in float32, the yardstick of tests/golden/make_operator_bounds.py attn.

Layout, as the kernels read it: qkv [rows, 3C] with head h at column 3 h dh as [q | k | v] (the oracle's view(.., heads, 3 dh).chunk(3),
oracle/sast_oracle.py:260); group m owns the K_m rows behind the exclusive prefix sum of Ks; o [rows, C]; lse [rows, heads].
tests/test_attn_reference.py pins this against the oracle lines it restates and against F.scaled_dot_product_attention.
"""
import math

import torch


def attention(qkv, Ks, dh):
    """per group and head: s = q k^T / sqrt(dh), lse = logsumexp(s), o = softmax(s) v  ->  (o [rows, C], lse [rows, heads])"""
    rows, C3 = qkv.shape
    C = C3 // 3
    heads = C // dh
    assert C3 == 3 * C and C == heads * dh and rows == sum(Ks)
    o, lse, r0 = [], [], 0
    for K in Ks:
        if K == 0:
            continue
        q, k, v = qkv[r0:r0 + K].view(K, heads, 3 * dh).transpose(0, 1).chunk(3, dim=2)      # (heads, K, dh) each
        s = q @ k.transpose(1, 2) / math.sqrt(dh)
        lse.append(torch.logsumexp(s, dim=2).t())
        o.append((torch.softmax(s, dim=2) @ v).transpose(0, 1).reshape(K, C))
        r0 += K
    return torch.cat(o), torch.cat(lse)


def logits(qkv, Ks, dh):
    """[(heads, K, K) scores of every kept group], for the conditions the cases are stated under"""
    heads = qkv.shape[1] // (3 * dh)
    out, r0 = [], 0
    for K in Ks:
        if K:
            q, k, _v = qkv[r0:r0 + K].view(K, heads, 3 * dh).transpose(0, 1).chunk(3, dim=2)
            out.append(q @ k.transpose(1, 2) / math.sqrt(dh))
        r0 += K
    return out


def split_qkv(t, dh):
    """[rows, 3C] in the kernels' column order -> (q, k, v), each [rows, heads, dh]"""
    rows, C3 = t.shape
    x = t.reshape(rows, C3 // (3 * dh), 3, dh)
    return x[:, :, 0], x[:, :, 1], x[:, :, 2]
