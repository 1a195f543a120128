"""The documented AdamW update (include/sast_hip.h: sast_adamw, sast_adamw_onecycle; torch.optim.AdamW semantics) restated in plain
torch, in any float dtype, over a list of gradients.  CPU only; independent of sast_amd.dist (tests/test_optim_reference.py compares it
with torch.optim.AdamW + OneCycleLR + clip_grad_value_ in float64, and with the torch-ops branch of FusedAdamW in float32).

Optimizer step t (1-based; t = t0 + 1 for the first gradient) with gradient g:
    g   <- g * grad_scale, THEN clipped by value to [-clip, clip] (clip <= 0: off)
    p   <- p * (1 - lr * wd)                                  decoupled decay
    m   <- b1 m + (1 - b1) g,   v <- b2 v + (1 - b2) g g
    p   <- p - lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
with both bias corrections evaluated in Python doubles, eps OUTSIDE the square root, and lr = lr_at(t - 1) under a schedule.
"""
import math

import torch


def onecycle_lr(step_num, max_lr, total_steps, pct_start=0.005, div_factor=25.0, final_div_factor=10000.0):
    """OneCycleLR, linear anneal, two phases, no momentum cycling, at scheduler step `step_num` (0-based).  The lr starts at
    max_lr / div_factor, reaches max_lr at step pct_start * total_steps - 1 and ends at max_lr / final_div_factor at step
    total_steps - 1.  Where the first phase ends before step 0 the second one runs from the start."""
    first, low = max_lr / div_factor, max_lr / final_div_factor
    end1, end2 = float(pct_start * total_steps) - 1.0, float(total_steps - 1)
    if step_num <= end1:
        return first + (max_lr - first) * (step_num / end1)
    return max_lr + (low - max_lr) * ((step_num - end1) / (end2 - end1))


def adamw(p0, grads, dtype, lr=None, schedule=None, betas=(0.9, 0.999), eps=1e-8, wd=0.0, grad_scale=1.0, clip=0.0, t0=0):
    """(p, m, v) after one step per gradient, from m = v = 0 at step count t0.  schedule: keyword arguments of `onecycle_lr`, else `lr`."""
    b1, b2 = betas
    p = p0.to(dtype).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for i, g in enumerate(grads):
        t = t0 + i + 1
        lr_t = onecycle_lr(t - 1, **schedule) if schedule is not None else lr
        g = g.to(dtype) * grad_scale
        if clip > 0:
            g = g.clamp(-clip, clip)
        p = p * (1 - lr_t * wd)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        denom = v.sqrt() / math.sqrt(1 - b2 ** t) + eps
        p = p - (lr_t / (1 - b1 ** t)) * (m / denom)
    return p, m, v
