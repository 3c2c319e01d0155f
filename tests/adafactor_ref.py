"""The DEFINITION of the Adafactor step of zett_amd.training.HypernetAdafactor / zett_op_adafactor_step, in float64 (no GPU):

    optax.chain(clip_by_global_norm(max_grad_norm),
                multi_transform({train: optax.adafactor(lr, weight_decay_rate=wd, weight_decay_mask=decay_mask_fn), freeze: set_to_zero}))

(the reference's train.py:631-656 with use_adafactor) with every other argument of optax.adafactor at its default:
min_dim_size_to_factor 128, decay_rate 0.8, decay_offset 0, multiply_by_parameter_scale, clipping_threshold 1.0, momentum None,
eps 1e-30.  optax is not a dependency of this project; the chain below restates its published source
(scale_by_factored_rms, clip_by_block_rms, scale_by_learning_rate, scale_by_param_block_rms, add_decayed_weights, in that order).

Per step, with t the number of updates applied so far:

  1. norm = l2 norm over every tensor that has a gradient, frozen ones included; coef = 1 if norm < max_grad_norm else
     max_grad_norm / norm (None: 1); g' = coef g.  A norm that is not finite: nothing changes (`skipped`).
  2. beta = 1 - (t + 1)^-0.8, the power taken in float64 and rounded to fp32 once (`decay`).
  3. q = g'^2 + 1e-30.  FACTORED (ndim == 2, smaller dimension >= 128), d0 the larger and d1 the smaller dimension by
     numpy.argsort(shape) (a square matrix: d1 = 0, d0 = 1):  v_row = beta v_row + (1 - beta) mean(q, d0)  [shape[d1] entries],
     v_col = beta v_col + (1 - beta) mean(q, d1)  [shape[d0] entries],  u = g' (v_row / mean(v_row))^-1/2 [along d0] v_col^-1/2 [along d1].
     Every other tensor:  v = beta v + (1 - beta) q,  u = g' v^-1/2.
  4. u_hat = u / max(1, sqrt(mean u^2)).
  5. s = sqrt(mean p^2) of the parameter before the update, 1e-3 where that is <= 1e-3.
  6. p <- p - (lr s u_hat + (wd p if the tensor decays else 0)).  The decay is NOT multiplied by lr: optax.adafactor adds the decayed
     weights after the learning-rate scaling.
"""
from __future__ import annotations

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
MIN_DIM_TO_FACTOR = 128
EPS, EPS_SCALE, CLIP, DECAY_RATE = 1e-30, 1e-3, 1.0, 0.8
DECAY, FROZEN = 1, 2              # zett_adamw_flags


def decay(t):
    """-> (beta, 1 - beta) of the step after t updates, as the fp32 values the device uses, in python floats"""
    pw = float(t + 1) ** -DECAY_RATE
    return float(torch.tensor(1.0 - pw, dtype=F64).to(F32)), float(torch.tensor(pw, dtype=F64).to(F32))


def factored_dims(shape):
    """-> None, or (d1, d0) = numpy.argsort(shape)[-2:] for a 2-D shape whose smaller dimension is >= 128"""
    if len(shape) != 2 or min(shape) < MIN_DIM_TO_FACTOR:
        return None
    order = np.argsort(np.asarray(shape), kind="stable")
    return int(order[-2]), int(order[-1])


def state_shapes(shape):
    dims = factored_dims(tuple(shape))
    if dims is None:
        return {"v": tuple(shape)}
    d1, d0 = dims
    return {"v_row": (shape[d1],), "v_col": (shape[d0],)}


def zero_state(shape):
    return {k: torch.zeros(s, dtype=F64) for k, s in state_shapes(shape).items()}


def global_norm(grads):
    return torch.sqrt(sum((g.to(F64) ** 2).sum() for g in grads)) if grads else torch.tensor(0.0, dtype=F64)


def clip_coef(norm, max_grad_norm):
    if max_grad_norm is None or float(norm) < max_grad_norm:
        return 1.0
    return float(max_grad_norm / norm)


def update_tensor(p, g, state, coef, beta, one_minus_beta, lr, wd):
    """One tensor of the `train` branch in float64.  -> (new p, new state, dict(u, rms_u, s))"""
    p, g = p.to(F64), g.to(F64)
    gp = coef * g
    q = gp * gp + EPS
    dims = factored_dims(tuple(p.shape))
    if dims is None:
        v = beta * state["v"].to(F64) + one_minus_beta * q
        u = gp * v ** -0.5
        new = {"v": v}
    else:
        d1, d0 = dims
        v_row = beta * state["v_row"].to(F64) + one_minus_beta * q.mean(d0)
        v_col = beta * state["v_col"].to(F64) + one_minus_beta * q.mean(d1)
        r = (v_row / v_row.mean()) ** -0.5
        c = v_col ** -0.5
        u = gp * r.unsqueeze(d0) * c.unsqueeze(d1)
        new = {"v_row": v_row, "v_col": v_col}
    rms_u = torch.sqrt((u * u).mean()) if u.numel() else torch.tensor(0.0, dtype=F64)
    u_hat = u / max(1.0, float(rms_u) / CLIP)
    s = float(torch.sqrt((p * p).mean())) if p.numel() else 0.0
    if s <= EPS_SCALE:
        s = EPS_SCALE
    return p - (lr * s * u_hat + wd * p), new, dict(u=u, rms_u=float(rms_u), s=s)


def step(params, grads, states, flags, t, lr, wd, max_grad_norm, coef=None, betas=None):
    """params / grads / states / flags: parallel lists (a frozen tensor's state is ignored and returned as it is).  coef / betas: the
    fp32 values a device record holds, to follow the device from exactly its scalars; None: computed here.
    -> dict(params, states, t, norm, coef, skipped)"""
    norm = global_norm(grads)
    if not bool(torch.isfinite(norm)):
        return dict(params=[p.to(F64) for p in params], states=states, t=t, norm=float(norm), coef=0.0, skipped=1)
    coef = clip_coef(norm, max_grad_norm) if coef is None else coef
    beta, omb = decay(t) if betas is None else betas
    out_p, out_s = [], []
    for p, g, st, fl in zip(params, grads, states, flags):
        if fl & FROZEN:
            out_p.append(p.to(F64))
            out_s.append(st)
            continue
        pn, sn, _ = update_tensor(p, g, st, coef, beta, omb, lr, wd if fl & DECAY else 0.0)
        out_p.append(pn)
        out_s.append(sn)
    return dict(params=out_p, states=out_s, t=t + 1, norm=float(norm), coef=coef, skipped=0)
